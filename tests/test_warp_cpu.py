"""Warp, host side (no GPU): the ABI of imm_warp_fit / imm_warp_u8 and their argument validation, the numpy restatements of the rule
against each other (tests/warp_reference.py), the host fit of imm_amd/warping.py, PhotoWarp.to_source and the refusals of plan_warp."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unalign_reference as UR                                              # noqa: E402
import warp_reference as R                                                  # noqa: E402

from imm_amd import warping as WP                                           # noqa: E402  (imports without a GPU)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ----------------------------------------------------------------------------------------------------------------------------
# ABI and validation
# ----------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_warp_entry_points():
    from imm_amd import _lib as L
    assert L.ABI_VERSION >= 30
    header = open(os.path.join(ROOT, 'include', 'imm_warp.h')).read()
    assert L.symbols('imm_warp.h') == ['imm_warp_fit', 'imm_warp_u8']
    for text in ('THE RULE', 'Frame.', 'Control points.', 'Fit (imm_warp_fit)', 'Warp (imm_warp_u8)', 'partial pivoting', 'rounded separately',
                 'logf', 'Identity.', 'links'):
        assert text in header, text
    src = open(os.path.join(ROOT, 'imm_amd', 'csrc', 'warp.hip')).read()
    assert 'fp contract(off)' in src and 'atomic' not in src.lower().replace('no atomics', '')


def test_warp_entry_points_validate_their_arguments_without_a_device():
    from imm_amd import _lib as L
    lib = L.load()
    one, two = C.c_void_p(16), C.c_void_p(32)              # non-null pointers that are never read: validation comes first
    nan, inf = float('nan'), float('inf')
    #       poses mu  anchors K   A  n  strength lam coef ctrl flags stream
    good = [one, one, one, 10, 8, 3, 1.0, 0.0, one, one, one, None]
    bad_args = [(i, None) for i in (0, 1, 2, 8, 9, 10)]
    bad_args += [(3, 0), (3, -1), (3, 73), (4, 7), (4, -4), (4, 72), (5, 0), (5, 65536), (5, -1)]
    bad_args += [(6, nan), (6, inf), (6, -inf), (7, nan), (7, inf), (7, -1e-9)]
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert lib.imm_warp_fit(*args) == -1, (i, bad)
        assert b'warp_fit' in lib.imm_last_error()
    assert lib.imm_warp_fit(one, one, one, 2, 0, 3, 1.0, 0.0, one, one, one, None) == -1          # anchors given at A == 0
    assert lib.imm_warp_fit(one, one, None, 2, 0, 3, 1.0, 0.0, one, one, one, None) == -1         # M == 2
    #       src  dst  offs hw  n_images boxes links ramp ctrl coef M  n  max_box_pixels stream
    good = [one, two, one, one, 2, one, one, one, one, one, 18, 3, 100, None]
    bad_args = [(i, None) for i in (0, 1, 2, 3, 5, 6, 7, 8, 9)]
    bad_args += [(1, one), (4, 0), (10, 2), (10, 81), (11, 0), (11, 65536), (12, 0), (12, -5)]
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert lib.imm_warp_u8(*args) == -1, (i, bad)
        assert b'warp_u8' in lib.imm_last_error()


def test_wrapper_refusals_come_before_any_device_call():
    from imm_amd import ops
    z = lambda *sh, **kw: torch.zeros(*sh, **kw)           # host tensors: a wrapper that got as far as the library would fault
    n, K, A = 2, 10, 8
    M = K + A
    poses, mu, anc, coef, ctrl, flags = z(n, K, 2), z(n, K, 2), z(A, 2), z(n, M + 3, 2), z(n, M, 2), z(n, dtype=torch.int32)
    for kw, match in ((dict(poses=z(n, K, 3)), 'poses'), (dict(mu=z(n, K + 1, 2)), 'mu'), (dict(mu=mu.double()), 'mu'),
                      (dict(anchors=z(A + 1, 2)), '3 <= K'), (dict(coef=z(n, M, 2)), 'coef'), (dict(ctrl=z(n, M + 3, 2)), 'ctrl'),
                      (dict(flags=z(n)), 'flags'), (dict(strength=float('nan')), 'strength'), (dict(lam=-1.0), 'lam'),
                      (dict(lam=float('inf')), 'lam'), (dict(poses=z(n, 2, 2), mu=z(n, 2, 2), anchors=None), '3 <= K'),
                      (dict(anchors=z(72, 2)), '3 <= K')):
        args = dict(poses=poses, mu=mu, anchors=anc, strength=1.0, lam=0.0, coef=coef, ctrl=ctrl, flags=flags)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.warp_fit(**args)
    src, dst, offs, hw = z(64, dtype=torch.uint8), z(64, dtype=torch.uint8), z(1, dtype=torch.int64), z(1, 2, dtype=torch.int32)
    boxes, links, ramp = z(n, 5, dtype=torch.int32), z(n, 2, dtype=torch.int32), z(n, 2)
    for kw, match in ((dict(src=src.float()), 'src'), (dict(dst=src), 'copy of src'), (dict(dst=z(32, dtype=torch.uint8)), 'copy of src'),
                      (dict(boxes=boxes.long()), 'boxes'), (dict(links=links[:1]), 'links'), (dict(inv_ramp=ramp.double()), 'inv_ramp'),
                      (dict(coef=z(n, M, 2)), 'coef'), (dict(ctrl=z(n, 2, 2)), 'control points'), (dict(hw=hw.long()), 'hw'),
                      (dict(max_box_pixels=0), 'max_box_pixels')):
        args = dict(src=src, dst=dst, offsets=offs, hw=hw, boxes=boxes, links=links, inv_ramp=ramp, ctrl=ctrl, coef=coef, max_box_pixels=9)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.warp_u8(**args)


# ----------------------------------------------------------------------------------------------------------------------------
# the rule
# ----------------------------------------------------------------------------------------------------------------------------
def test_anchors_and_control_points():
    assert WP.warp_anchors(0).shape == (0, 2)
    assert WP.warp_anchors(1).tolist() == [[-1, -1], [-1, 1], [1, 1], [1, -1]]
    assert WP.warp_anchors(2).tolist() == [[-1, -1], [-1, 0], [-1, 1], [0, 1], [1, 1], [1, 0], [1, -1], [0, -1]]
    for m in range(0, 7):
        a = WP.warp_anchors(m)
        assert np.array_equal(a, R.anchors(m)) and a.shape == (4 * m, 2) and len({tuple(p) for p in a.tolist()}) == 4 * m
        assert m == 0 or (np.abs(a).max(axis=1) == 1.0).all()                      # on the border
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match='anchors'):
            WP.warp_anchors(bad)
    poses = np.random.RandomState(0).uniform(-1, 1, (3, 5, 2))
    c = WP.control_points(poses, 2)
    assert c.dtype == F32 and c.shape == (3, 13, 2) and np.array_equal(c, R.control(poses, 2))
    assert np.array_equal(c[:, :5], poses.astype(F32)) and np.array_equal(c[1, 5:], WP.warp_anchors(2).astype(F32))


@pytest.mark.parametrize('K,m', R.KERNEL_SHAPES)
def test_host_fit_is_the_restatement_and_interpolates(K, m):
    _photos, rows, mu, poses = R.kernel_case(K, m)
    M = K + 4 * m
    for lam in R.LAMS:
        coef, ctrl, flags = WP.fit_warp(poses, mu, m, 1.0, lam)
        want, want_ctrl, want_flags, cond = R.fit_f64(poses, mu, m, 1.0, lam)
        good = np.nonzero(want_flags == 0)[0]
        assert np.array_equal(flags, want_flags) and flags.tolist() == [int(b == R.NAN_ROW) for b in range(len(rows))]
        assert np.array_equal(ctrl[good], want_ctrl[good]) and np.isnan(coef[R.NAN_ROW]).all()
        assert np.allclose(coef[good], want[good], rtol=1e-9, atol=1e-12)
        # the condition numbers the GPU fit test's bound relies on
        print('\nWARP FIT K=%d anchors=%d lam=%g: condition numbers %.3g .. %.3g' % (K, m, lam, cond[good].min(), cond[good].max()))
        assert cond[good].max() <= 1e4
        # poses == mu: a zero right-hand side eliminates to exactly zero coefficients
        assert not coef[R.IDENTITY_ROW].any()
        if lam == 0.0:
            for b in good:
                D = WP.displacement(coef[b], ctrl[b], ctrl[b])
                assert np.abs(D[:K] - (mu[b].astype(np.float64) - poses[b].astype(np.float64))).max() < 1e-10
                assert M == K or np.abs(D[K:]).max() < 1e-10
    half = WP.fit_warp(poses, mu, m, 0.5, 0.0)[0]
    good = [b for b in range(len(rows)) if b != R.NAN_ROW]
    assert np.allclose(half[good], 0.5 * WP.fit_warp(poses, mu, m, 1.0, 0.0)[0][good], rtol=1e-9, atol=1e-13)


def test_host_fit_flags_rows_without_an_answer():
    rng = np.random.RandomState(5)
    mu, poses = R.landmarks(10, 4, rng)
    poses[1, 3] = poses[1, 7]                              # coincident control points at lam == 0: singular
    poses[2, 0, 0] = np.inf
    mu[3, 9, 1] = np.nan
    coef, _ctrl, flags = WP.fit_warp(poses, mu, 2, 1.0, 0.0)
    assert flags.tolist() == [0, 1, 1, 1] and np.isfinite(coef[0]).all() and np.isnan(coef[1:]).all()
    assert R.fit_f64(poses, mu, 2, 1.0, 0.0)[2].tolist() == [0, 1, 1, 1]
    assert WP.fit_warp(poses, mu, 2, 1.0, 1e-2)[2].tolist() == [0, 0, 1, 1]      # smoothing lifts the coincidence


@pytest.mark.parametrize('K,m', R.KERNEL_SHAPES)
def test_f32_restatement_against_f64(K, m):
    """The committed seed: warp_f32 against warp_f64, both driven by the f32-rounded coefficients, differs by at most one grey level on
    at most HALF the cap's share (0.25 % of the covered pixels), for every lam and feather of the GPU parity test: the other half is
    left to the device's log."""
    photos, rows, mu, poses = R.kernel_case(K, m)
    for lam in R.LAMS:
        coef, ctrl, flags, _cond = R.fit_f64(poses, mu, m, 1.0, lam)
        coef32 = coef.astype(F32)
        for feather in R.FEATHERS:
            ramp = R.inv_ramp(rows, feather)
            ref64, covered = R.warp_f64(photos, rows, ctrl, coef32, ramp)
            ref32 = R.warp_f32(photos, rows, ctrl, coef32, ramp)
            n_diff, worst, _near, n_cov = UR.within_cap(ref32, ref64, covered, R.no_band(photos))
            print('\nWARP f32 vs f64 K=%d anchors=%d lam=%g feather=%g: %d of %d covered pixels differ (max %d)' % (
                K, m, lam, feather, n_diff, n_cov, worst))
            assert n_diff <= 0.0025 * n_cov
            # what no row covers is the input's; the flagged row, the rows without a photo and the box outside write nothing
            for p, o, cov in zip(photos, ref32, covered):
                assert np.array_equal(o[~cov], p[~cov])
            assert not covered[3].any() and sum(int(c.sum()) for c in covered) > 1500
            changed = sum(int((o != p).any(axis=2).sum()) for o, p in zip(ref32, photos))
            assert changed > 0.3 * n_cov, 'the warp moves pixels'
    # the identity row alone returns its photo bit for bit
    one = rows[R.IDENTITY_ROW:R.IDENTITY_ROW + 1]
    for feather in R.FEATHERS:
        same = R.warp_f32(photos, one, ctrl[:1], coef32[:1], R.inv_ramp(one, feather))
        assert all(np.array_equal(a, b) for a, b in zip(same, photos))


def test_translation_shifts_the_box_interior():
    """anchors = 0, lam = 0, poses = mu + (2 * 3 / H, -2 * 2 / W): the spline is the constant displacement and, with feather 0, the box
    holds the photo shifted by (3, -2) pixels, edge-clamped, bit for bit."""
    rng = np.random.RandomState(3)
    photo = rng.randint(0, 256, size=(48, 56, 3)).astype(np.uint8)
    rows = np.array([(0, 4, 20, 36, 52), (0, 30, -8, 62, 24)], dtype=np.int32)              # 32 x 32 boxes: every value exact in f32
    mu = (rng.randint(-40, 41, size=(2, 6, 2)) / 64.0).astype(F32)
    poses = (mu + np.array([6.0 / 32.0, -4.0 / 32.0], dtype=F32)).astype(F32)
    coef, ctrl, flags = WP.fit_warp(poses, mu, 0, 1.0, 0.0)
    assert not flags.any() and np.abs(coef[:, :6]).max() < 1e-12 and np.allclose(coef[:, 6], [-6.0 / 32.0, 4.0 / 32.0])
    for b in range(2):
        got = R.warp_f32([photo], rows[b:b + 1], ctrl[b:b + 1], coef[b:b + 1].astype(F32), R.inv_ramp(rows[b:b + 1], 0.0))[0]
        assert np.array_equal(got, R.shifted(photo, rows[b], 3, -2))


# ----------------------------------------------------------------------------------------------------------------------------
# plan_warp and PhotoWarp
# ----------------------------------------------------------------------------------------------------------------------------
def test_plan_warp_refusals():
    photos = [np.zeros((40, 50, 3), np.uint8), np.zeros((30, 30, 3), np.uint8)]
    K = 10
    _mu, poses = R.landmarks(K, 2, np.random.RandomState(1))
    plan = WP.plan_warp(photos, poses, None, None, 0.125, K)
    assert plan[1].tolist() == [[0, 0, 0, 40, 50], [1, 0, 0, 30, 30]] and plan[2][0] == 'landmarks' and plan[4:] == (2, 0.0, 1.0, 18)
    assert WP.plan_warp(photos, poses[:1], [(1, 2, 2, 20, 20)] * 3, None, 0.0, K, anchors=0)[7] == 10
    pose_photos = [np.zeros((20, 20, 3), np.uint8)]
    assert WP.plan_warp(photos, pose_photos, None, None, 0.5, K)[2][0] == 'photos'
    close = poses.copy()
    close[1, 4] = close[1, 2] + F32(5e-7)
    on_anchor = poses.copy()
    on_anchor[0, 3] = (-1.0, 0.0)
    for args, kw, match in (((photos, close, None, None, 0.125, K), {}, 'pose 1: control points 2 and 4'),
                            ((photos, on_anchor, None, None, 0.125, K), {}, 'pose 0: control points 3 and 11'),
                            ((photos, poses[:, :2], None, None, 0.125, 2), dict(anchors=0), '>= 3 control points'),
                            ((photos, poses, None, None, 0.125, K), dict(anchors=18), '<= 80 control points'),
                            ((photos, poses, None, None, 0.125, K), dict(anchors=-1), 'anchors'),
                            ((photos, poses, None, None, 0.125, K), dict(anchors=1.5), 'anchors'),
                            ((photos, poses, None, None, 0.125, K), dict(lam=-0.1), 'lam'),
                            ((photos, poses, None, None, 0.125, K), dict(lam=float('nan')), 'lam'),
                            ((photos, poses, None, None, 0.125, K), dict(strength=float('inf')), 'strength'),
                            ((photos, poses, None, None, 0.75, K), {}, 'feather'),
                            ((photos, poses[:, :9], None, None, 0.125, K), {}, 'poses must be landmarks'),
                            ((photos, poses, [(0, 0, 0, 10, 10)], None, 0.125, K), {}, 'poses must be landmarks'),
                            ((photos, poses, None, [(0, 0, 0, 10, 10)], 0.125, K), {}, 'pose_boxes'),
                            ((torch.zeros(2, 128, 128, 3), poses, None, None, 0.125, K), {}, 'u8 arrays')):
        with pytest.raises(ValueError, match=match):
            WP.plan_warp(*args, **kw)
    nan = poses.copy()
    nan[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match='finite'):
        WP.plan_warp(photos, nan, None, None, 0.125, K)


@pytest.mark.parametrize('m', [0, 2])
def test_photo_warp_to_source(m):
    """T(p_k) = mu_k at lam = 0, in photo pixels; with anchors, the anchor points of the box border map to themselves."""
    K = 10
    rng = np.random.RandomState(2)
    mu, poses = R.landmarks(K, 3, rng)
    rows = np.array([(0, 10, 20, 110, 140), (1, -5, -5, 60, 45), (0, 0, 0, 33, 77)], dtype=np.int32)
    coef, ctrl, flags = WP.fit_warp(poses, mu, m, 1.0, 0.0)
    pw = WP.PhotoWarp(coef.astype(F32), ctrl, rows, mu, poses, flags, 1.0, 0.0, m)
    org, half = rows[:, None, 1:3].astype(np.float64), (rows[:, None, 3:5] - rows[:, None, 1:3]) / 2.0
    to_px = lambda q: org + (np.asarray(q, np.float64) + 1.0) * half
    got = pw.to_source(to_px(poses))
    assert got.shape == (3, K, 2) and got.dtype == np.float64
    # f32 coefficients: |error| <= 2^-24 sum_j |U_j w_j| H / 2 and the like for the affine part; 1e-4 px is far above that here
    assert np.abs(got - to_px(mu)).max() < 1e-4
    exact = WP.PhotoWarp(coef, ctrl, rows, mu, poses, flags, 1.0, 0.0, m).to_source(to_px(poses))
    assert np.abs(exact - to_px(mu)).max() < 1e-9
    if m:
        border = np.broadcast_to(to_px(WP.warp_anchors(m)[None]), (3, 4 * m, 2))
        assert np.abs(pw.to_source(border) - border).max() < 1e-4
        assert np.abs(WP.PhotoWarp(coef, ctrl, rows, mu, poses, flags, 1.0, 0.0, m).to_source(border) - border).max() < 1e-9
    with pytest.raises(ValueError, match='points_px'):
        pw.to_source(np.zeros((2, 4, 2)))
    # strength 0: the identity map
    zero = WP.fit_warp(poses, mu, m, 0.0, 0.0)[0]
    pts = rng.uniform(0, 100, (3, 7, 2))
    assert np.array_equal(WP.PhotoWarp(zero, ctrl, rows, mu, poses, flags, 0.0, 0.0, m).to_source(pts), pts)
