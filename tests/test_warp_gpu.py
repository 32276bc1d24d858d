"""Warp on the MI355X: imm_warp_fit against numpy's f64 solution, imm_warp_u8 within the cap of the f64 restatement of the rule
(tests/warp_reference.py) driven by the kernel's own coefficients, the identity and the translation bit for bit, invariance under
splitting a call into launches, guarded buffers, and LandmarkDetector.warp with the script."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compose_reference as CR                                               # noqa: E402
import guarded                                                               # noqa: E402
import unalign_reference as UR                                               # noqa: E402
import warp_reference as R                                                   # noqa: E402
from alignment_reference import smooth_photo                                  # noqa: E402
from dataset_fixtures import make_celeba_tree                                 # noqa: E402
from test_detector_gpu import _run_script, _write_config                      # noqa: E402
from test_generator_gpu import make_model as make_generator_model             # noqa: E402
from test_unalign_gpu import SURFACE_BOXES, SURFACE_SIZES                     # noqa: E402

from imm_amd import generation as G                                           # noqa: E402
from imm_amd import warping as WP                                             # noqa: E402
from imm_amd.inference import plan_buckets                                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 128
F32 = np.float32


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


def dev(ops, a):
    return ops.to_device_pinned(np.ascontiguousarray(a), DEV)


def run_fit(ops, poses, mu, m, strength=1.0, lam=0.0):
    """imm_warp_fit in guarded buffers -> (coef f32 [n, M + 3, 2], ctrl f32 [n, M, 2], flags int32 [n]) as host arrays."""
    n, K = poses.shape[:2]
    M = K + 4 * m
    guarded.reset()
    coef = guarded.out((n, M + 3, 2), torch.float32, DEV)
    ctrl = guarded.out((n, M, 2), torch.float32, DEV)
    flags = guarded.out((n,), torch.int32, DEV)
    anc = guarded.inp(torch.from_numpy(WP.warp_anchors(m).astype(F32)), DEV) if m else None
    ops.warp_fit(guarded.inp(torch.from_numpy(np.ascontiguousarray(poses)), DEV), guarded.inp(torch.from_numpy(np.ascontiguousarray(mu)), DEV),
                 anc, strength, lam, coef, ctrl, flags)
    torch.cuda.synchronize()
    guarded.check_guards()
    return coef.cpu().numpy(), ctrl.cpu().numpy(), flags.cpu().numpy()


def run_warp(ops, photos, rows, ctrl, coef, feather, launches=None, links=None, max_pixels=None):
    """imm_warp_u8 over the packed photos, source and canvas in guarded buffers, the rows issued as the given launches (lists of
    consecutive row indices, in order; default: one launch of all rows), the grid sized by max_pixels (default: the launch's largest box).
    Returns (the whole canvas as a host array, the packed input)."""
    buf, offs, hw = CR.pack(photos)
    guarded.reset()
    src = guarded.inp(torch.from_numpy(buf), DEV)
    canvas = guarded.out(buf.shape, torch.uint8, DEV, fill=torch.from_numpy(buf))
    offs_d, hw_d = dev(ops, offs), dev(ops, hw)
    ctrl_d, coef_d = guarded.inp(torch.from_numpy(np.ascontiguousarray(ctrl, F32)), DEV), guarded.inp(torch.from_numpy(np.ascontiguousarray(coef, F32)), DEV)
    ramp = R.inv_ramp(rows, feather)
    assert np.array_equal(ramp, G.compose_inv_ramp(rows, feather))
    for part in ([list(range(len(rows)))] if launches is None else launches):
        assert part == list(range(part[0], part[-1] + 1))
        sl = slice(part[0], part[-1] + 1)
        sub = rows[sl]
        area = int(max(1, ((sub[:, 3] - sub[:, 1]) * (sub[:, 4] - sub[:, 2])).max())) if max_pixels is None else max_pixels
        lk = G.compose_links(sub) if links is None else links[sl]
        ops.warp_u8(src, canvas, offs_d, hw_d, dev(ops, sub), dev(ops, lk), dev(ops, ramp[sl]), ctrl_d[sl], coef_d[sl], area)
    torch.cuda.synchronize()
    guarded.check_guards()
    assert np.array_equal(src.cpu().numpy(), buf), 'the source buffer is read only'
    return canvas.cpu().numpy(), buf


def ulp32(x):
    """The f32 spacing at |x| (at least the smallest normal's)."""
    return np.spacing(np.maximum(np.abs(x), np.finfo(F32).tiny).astype(F32)).astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the fit
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,m', R.KERNEL_SHAPES)
def test_warp_fit_kernel(ops, K, m):
    """Every coefficient within one f32 ulp of numpy's f64 solution plus 1e-9 x the column's largest magnitude: the kernel's only
    rounding of consequence is the final f32 store (half an ulp); its f64 elimination, at condition numbers <= 1e4 (asserted in
    test_warp_cpu), stays below 1e4 x 2^-52 x a modest growth factor, orders under 1e-9."""
    _photos, rows, mu, poses = R.kernel_case(K, m)
    for lam in R.LAMS:
        for strength in (1.0, 0.5):
            coef, ctrl, flags = run_fit(ops, poses, mu, m, strength, lam)
            want, want_ctrl, want_flags, cond = R.fit_f64(poses, mu, m, strength, lam)
            good = np.nonzero(want_flags == 0)[0]
            assert np.array_equal(flags, want_flags) and flags[R.NAN_ROW] == 1 and flags.sum() == 1
            assert np.array_equal(ctrl.view(np.uint32), want_ctrl.view(np.uint32)), 'ctrl is not (poses, anchors), bit for bit'
            assert np.isnan(coef[R.NAN_ROW]).all() and np.isfinite(coef[good]).all()
            tol = ulp32(want[good]) + 1e-9 * np.abs(want[good]).max(axis=1, keepdims=True)
            err = np.abs(coef[good].astype(np.float64) - want[good])
            print('\nWARP FIT K=%d anchors=%d lam=%g strength=%g: max err / tol %.3g (cond <= %.3g)' % (
                K, m, lam, strength, (err / tol).max(), cond[good].max()))
            assert (err <= tol).all()
            assert not coef[R.IDENTITY_ROW].any(), 'poses == mu must give exactly zero coefficients'
            host = WP.fit_warp(poses, mu, m, strength, lam)[0]
            assert (np.abs(coef[good].astype(np.float64) - host[good]) <= tol).all()


def test_warp_fit_flags_rows_without_an_answer(ops):
    rng = np.random.RandomState(5)
    mu, poses = R.landmarks(10, 5, rng)
    poses[1, 3] = poses[1, 7]                              # coincident control points at lam == 0: an exactly zero pivot
    poses[2, 0, 0] = np.inf
    mu[3, 9, 1] = np.nan
    poses[4, 2] = (1.0, 0.0)                               # a landmark on an anchor
    for m, want in ((2, [0, 1, 1, 1, 1]), (0, [0, 1, 1, 1, 0])):
        coef, _ctrl, flags = run_fit(ops, poses, mu, m)
        assert flags.tolist() == want == WP.fit_warp(poses, mu, m)[2].tolist()
        bad = np.array(want, dtype=bool)
        assert np.isnan(coef[bad]).all() and np.isfinite(coef[~bad]).all()
    assert run_fit(ops, poses, mu, 2, lam=1e-2)[2].tolist() == [0, 0, 1, 1, 0]              # smoothing lifts the coincidences
    # three points on one line: no affine part
    line = np.array([[[-0.5, -0.5], [0.0, 0.0], [0.25, 0.25]]], dtype=F32)
    assert run_fit(ops, line, line + F32(0.125), 0)[2].tolist() == [1]


# ----------------------------------------------------------------------------------------------------------------------------
# 2. the warp: parity and guards, 3. identity, 4. translation, 5. split invariance
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('feather', R.FEATHERS)
@pytest.mark.parametrize('K,m', R.KERNEL_SHAPES)
def test_warp_kernel_parity(ops, K, m, feather):
    photos, rows, mu, poses = R.kernel_case(K, m)
    for lam in R.LAMS:
        coef, ctrl, flags = run_fit(ops, poses, mu, m, 1.0, lam)
        got, buf = run_warp(ops, photos, rows, ctrl, coef, feather)
        ramp = R.inv_ramp(rows, feather)
        ref64, covered = R.warp_f64(photos, rows, ctrl, coef, ramp)
        ref32 = R.warp_f32(photos, rows, ctrl, coef, ramp)
        out = CR.unpack(got, photos)
        n32 = sum(int((a != b).any(axis=2).sum()) for a, b in zip(out, ref32))
        d64 = [np.abs(a.astype(int) - b.astype(int)).max(axis=2) for a, b in zip(out, ref64)]
        print('\nWARP KERNEL K=%d anchors=%d lam=%g feather=%g: %d of %d covered pixels differ from the f64 restatement (max %d), %d from '
              'the f32 one' % (K, m, lam, feather, sum(int((d > 0).sum()) for d in d64), sum(int(c.sum()) for c in covered),
                               max(int(d.max()) for d in d64), n32))
        UR.within_cap(out, ref64, covered, R.no_band(photos))
        # every byte no row writes - other pixels, the photo without a row, the padding between photos - is the input's; the flagged
        # row, the rows without a photo and the box outside its photo write nothing
        inside, _o, _h = CR.pack([np.repeat(c[:, :, None], 3, axis=2).astype(np.uint8) for c in covered])
        inside = inside == 1                                                  # (the padding of that buffer holds 0xA5)
        assert inside.sum() == 3 * sum(int(c.sum()) for c in covered) and not covered[3].any()
        assert np.array_equal(got[~inside], buf[~inside])
        y0, x0, y1, x1 = rows[R.NAN_ROW, 1:]
        assert flags[R.NAN_ROW] == 1 and not covered[rows[R.NAN_ROW, 0]][y0:y1, x0:x1].any()
        changed = sum(int((o != p).any(axis=2).sum()) for o, p in zip(out, photos))
        assert changed > 0.3 * sum(int(c.sum()) for c in covered), 'the warp moves pixels'


@pytest.mark.parametrize('K,m', [(10, 0), (10, 2), (64, 4)])
def test_warp_identity(ops, K, m):
    """Rows with poses == mu return the photo bit for bit, for every feather and with and without anchors."""
    photos, rows, mu, poses = R.kernel_case(K, m)
    mu[R.NAN_ROW] = poses[R.NAN_ROW]
    coef, ctrl, flags = run_fit(ops, poses, poses, m)
    assert not flags.any() and not coef.any()
    for feather in R.FEATHERS + (0.25,):
        got, buf = run_warp(ops, photos, rows, ctrl, coef, feather)
        assert np.array_equal(got, buf), feather
    # and the warp is no no-op: the case's own landmarks move the boxes
    coef, ctrl, _flags = run_fit(ops, poses, mu, m)
    got, buf = run_warp(ops, photos, rows, ctrl, coef, 0.25)
    assert not np.array_equal(got, buf)


def test_warp_translation(ops):
    """anchors = 0, lam = 0, poses = mu + (2 * 3 / H, -2 * 2 / W), feather 0: the box holds the photo shifted by (3, -2) pixels,
    edge-clamped, bit for bit (32 x 32 boxes and landmarks on a 1 / 64 grid: every value is exact in f32)."""
    rng = np.random.RandomState(3)
    photo = rng.randint(0, 256, size=(48, 56, 3)).astype(np.uint8)
    rows = np.array([(0, 4, 20, 36, 52), (0, 30, -8, 62, 24)], dtype=np.int32)
    mu = (rng.randint(-40, 41, size=(2, 6, 2)) / 64.0).astype(F32)
    poses = (mu + np.array([6.0 / 32.0, -4.0 / 32.0], dtype=F32)).astype(F32)
    coef, ctrl, flags = run_fit(ops, poses, mu, 0)
    assert not flags.any() and np.abs(coef[:, :6]).max() < 1e-12 and np.array_equal(coef[:, 6], np.tile(F32([-0.1875, 0.125]), (2, 1)))
    for b in range(2):
        got, _buf = run_warp(ops, [photo], rows[b:b + 1], ctrl[b:b + 1], coef[b:b + 1], 0.0)
        assert np.array_equal(CR.unpack(got, [photo])[0], R.shifted(photo, rows[b], 3, -2)), b


def test_warp_split_invariance(ops):
    photos, rows, mu, poses = R.kernel_case(10, 2)
    coef, ctrl, _flags = run_fit(ops, poses, mu, 2)
    n = len(rows)
    for feather in (0.0, 0.125):
        one, _ = run_warp(ops, photos, rows, ctrl, coef, feather)
        two, _ = run_warp(ops, photos, rows, ctrl, coef, feather, [list(range(0, 4)), list(range(4, n))])
        each, _ = run_warp(ops, photos, rows, ctrl, coef, feather, [[i] for i in range(n)])
        assert np.array_equal(one, two) and np.array_equal(one, each), feather
    # the two-launch split parts the three mutually overlapping rows, and their order matters
    assert sum(i < 4 for i in R.OVERLAPPING) == 1
    ramp = R.inv_ramp(rows, 0.0)
    fwd = R.warp_f32(photos, rows, ctrl, coef, ramp)
    order = [i for i in range(n) if i not in R.OVERLAPPING] + list(R.OVERLAPPING)[::-1]
    rev = R.warp_f32(photos, rows[order], ctrl[order], coef[order], ramp[order])
    assert not all(np.array_equal(a, b) for a, b in zip(fwd, rev))


def test_warp_one_block_per_row(ops):
    """The grid-size argument set to 1: ONE block of 256 threads per row carries every box through the grid-stride loop, and the bytes
    are those of a grid as large as the largest box."""
    photos, rows, mu, poses = R.kernel_case(10, 2)
    coef, ctrl, _flags = run_fit(ops, poses, mu, 2)
    assert ((rows[:, 3] - rows[:, 1]) * (rows[:, 4] - rows[:, 2])).max() > 2 * 256
    for feather in (0.0, 0.125):
        full, _ = run_warp(ops, photos, rows, ctrl, coef, feather)
        one, _ = run_warp(ops, photos, rows, ctrl, coef, feather, max_pixels=1)
        assert np.array_equal(one, full), feather


# ----------------------------------------------------------------------------------------------------------------------------
# 6. guards: whatever the device buffers hold, nothing outside the packed buffers is addressed
# ----------------------------------------------------------------------------------------------------------------------------
def test_warp_addresses_nothing_outside_the_photos(ops):
    photos, rows, mu, poses = R.kernel_case(10, 2)
    coef, ctrl, _flags = run_fit(ops, poses, mu, 2)
    rng = np.random.RandomState(9)
    n = len(rows)
    wild = coef.copy()
    wild[1::4] *= F32(1e6)                                  # samples far outside the photo: clamped to its edge
    wild[2::4] *= F32(1e30)                                 # beyond what an int holds
    wild[3::4, 5] = np.inf
    wild[0, 2, 1] = np.nan
    links = rng.randint(-5, n + 5, size=(n, 2)).astype(np.int32)             # chains that loop, leave [0, n) and join other photos
    for lk in (None, links):
        got, buf = run_warp(ops, photos, rows, ctrl, wild, 0.125, links=lk)    # run_warp checks the guard bands of every buffer
        boxes = CR.box_mask(photos, rows[[b for b in range(n) if 0 <= rows[b, 0] < len(photos)]])
        inside, _o, _h = CR.pack([np.repeat(c[:, :, None], 3, axis=2).astype(np.uint8) for c in boxes])
        assert np.array_equal(got[inside != 1], buf[inside != 1])
    # a row of NaN coefficients writes nothing at all
    nan = np.full_like(coef, np.nan)
    got, buf = run_warp(ops, photos, rows, ctrl, nan, 0.0)
    assert np.array_equal(got, buf)


# ----------------------------------------------------------------------------------------------------------------------------
# 7. LandmarkDetector.warp
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def m128(ops):
    return make_generator_model(10, S, 4)


@pytest.fixture(scope='module')
def scene():
    """Seven rows over six photos, one overlap, two buckets at max_batch = 4 (test_unalign_gpu's scene).  The poses lie on a jittered
    grid: they are the splines' control points, and an untrained model's own landmarks sit in a small cloud, whose systems are too
    ill-conditioned (condition numbers near 1e7) for an f32 evaluation to stay within the cap."""
    ims = [smooth_photo(h, w, 60 + i) for i, (h, w) in enumerate(SURFACE_SIZES)]
    _mu, poses = R.landmarks(10, len(SURFACE_BOXES), np.random.RandomState(12))
    return ims, poses


def test_detector_warp_against_the_restatement(m128, scene):
    from imm_amd import keypoints as KP
    from imm_amd.inference import LandmarkDetector
    cfg, model, eng, P, St = m128
    ims, poses = scene
    det = model.landmark_detector(S, max_batch=4)
    assert len(plan_buckets(len(SURFACE_BOXES), 4)) == 2
    rows = KP.check_boxes(SURFACE_BOXES, len(ims))
    mu = det.landmarks(ims, SURFACE_BOXES)
    for feather, m, lam in ((0.125, 2, 0.0), (0.0, 0, 1e-2)):
        out, pw = det.warp(ims, poses, SURFACE_BOXES, feather=feather, anchors=m, lam=lam, return_transform=True)
        torch.cuda.synchronize()
        assert isinstance(pw, WP.PhotoWarp) and (pw.anchors, pw.lam, pw.strength) == (m, lam, 1.0) and np.array_equal(pw.rows, rows)
        assert torch.equal(pw.mu, mu) and torch.equal(pw.poses.cpu(), torch.from_numpy(poses)) and not pw.flags.any()
        coef, ctrl = pw.coef.cpu().numpy(), pw.ctrl.cpu().numpy()
        assert coef.shape == (7, 10 + 4 * m + 3, 2) and np.array_equal(ctrl, WP.control_points(poses, m))
        want, _c, _f, cond = R.fit_f64(poses, mu.cpu().numpy(), m, 1.0, lam)
        assert (np.abs(coef - want) <= ulp32(want) + 1e-9 * np.abs(want).max(axis=1, keepdims=True)).all() and cond.max() <= 1e4
        ref64, covered = R.warp_f64(ims, rows, ctrl, coef, R.inv_ramp(rows, feather))
        got = [o.cpu().numpy() for o in out]
        for o, im in zip(out, ims):
            assert o.dtype == torch.uint8 and o.device.type == 'cuda' and tuple(o.shape) == im.shape
        n_diff, worst, _near, n_cov = UR.within_cap(got, ref64, covered, R.no_band(ims))
        changed = sum(int((g != im).any(axis=2).sum()) for g, im in zip(got, ims))
        print('\nWARP() feather=%g anchors=%d lam=%g: %d of %d covered pixels differ from the f64 restatement (max %d), %d changed' % (
            feather, m, lam, n_diff, n_cov, worst, changed))
        assert changed > 0.3 * n_cov and all(np.array_equal(g[~c], im[~c]) for g, im, c in zip(got, ims, covered))
        # a second call gives the same bytes and leaves the first call's result alone; plain launches give them too
        before = [o.clone() for o in out]
        again = det.warp(ims, poses, SURFACE_BOXES, feather=feather, anchors=m, lam=lam)
        assert all(torch.equal(x, y) for x, y in zip(before, again)) and all(torch.equal(x, y) for x, y in zip(before, out))
        if lam == 0.0:
            # T(p_k) = mu_k: |to_source(poses in px) - mu in px| within four times the f32 rounding bound of the coefficients,
            # 2^-23 sum_j |U_j w_j| H / 2, computed from the f64 solution
            geom = KP.box_geometry(rows, S).astype(np.float64)
            to_px = lambda q: KP.to_source_pixels((np.asarray(q, np.float64) + 1.0) * (S / 2.0), geom)
            err = np.abs(pw.to_source(to_px(poses)) - to_px(mu.cpu().numpy()))
            bound = np.empty_like(err)
            for b in range(7):
                d = ctrl[b, :10, None, :].astype(np.float64) - ctrl[b, None, :, :].astype(np.float64)
                u = np.abs(R.U((d * d).sum(axis=-1)))                          # [k, j]
                half = (rows[b, 3:5] - rows[b, 1:3]) / 2.0
                bound[b] = 4.0 * 2.0 ** -23 * (u @ np.abs(want[b, :10 + 4 * m])) * half
            print('WARP() to_source: max |T(p_k) - mu_k| %.3g px, max err / bound %.3g' % (err.max(), (err / bound).max()))
            assert (err <= bound).all()
    plain = LandmarkDetector(model, S, max_batch=4, use_graph=False)
    assert all(torch.equal(x, y) for x, y in zip(plain.warp(ims, poses, SURFACE_BOXES, feather=0.0, anchors=0, lam=1e-2), out))
    # strength 0 and poses == mu: the photos themselves
    for same in (det.warp(ims, poses, SURFACE_BOXES, strength=0.0), det.warp(ims, mu, SURFACE_BOXES), det.warp(ims, mu, SURFACE_BOXES, anchors=0)):
        assert all(np.array_equal(o.cpu().numpy(), im) for o, im in zip(same, ims))
    # pose photos against explicit landmarks; one pose for every row; whole-photo boxes by default
    pose_photos = [smooth_photo(150, 140, 31 + i) for i in range(7)]
    lm = det.landmarks(pose_photos)
    # (an untrained model's landmarks are a small cloud: lam keeps those systems usable)
    a = det.warp(ims, pose_photos, SURFACE_BOXES, lam=1.0)
    b = det.warp(ims, lm, SURFACE_BOXES, lam=1.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not all(np.array_equal(x.cpu().numpy(), im) for x, im in zip(a, ims))
    a = det.warp(ims, pose_photos[:1], SURFACE_BOXES, pose_boxes=[(0, 10, 10, 140, 130)], lam=1.0)
    b = det.warp(ims, det.landmarks(pose_photos[:1], [(0, 10, 10, 140, 130)]), SURFACE_BOXES, lam=1.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    whole = det.warp(ims, poses[:6])
    assert len(whole) == 6 and all(tuple(o.shape) == im.shape for o, im in zip(whole, ims))
    # the photos handed in are not written
    assert all(np.array_equal(im, smooth_photo(h, w, 60 + i)) for i, (im, (h, w)) in enumerate(zip(ims, SURFACE_SIZES)))


def test_detector_warp_refusals(m128, scene):
    cfg, model, eng, P, St = m128
    ims, poses = scene
    det = model.landmark_detector(S, max_batch=4)
    close = poses.copy()
    close[2, 1] = close[2, 8]
    for kw, match in ((dict(feather=0.75), 'feather'), (dict(anchors=18), '<= 80 control points'), (dict(anchors=-2), 'anchors'),
                      (dict(lam=-1.0), 'lam'), (dict(lam=float('nan')), 'lam'), (dict(strength=float('inf')), 'strength'),
                      (dict(poses=close), 'pose 2: control points 1 and 8'), (dict(poses=poses[:3]), 'poses must be landmarks'),
                      (dict(pose_boxes=[(0, 0, 0, 5, 5)]), 'pose_boxes'), (dict(photos=torch.zeros(6, S, S, 3)), 'u8 arrays'),
                      (dict(boxes=[(9, 0, 0, 5, 5)] * 7), 'names image')):
        args = dict(photos=ims, poses=poses, boxes=SURFACE_BOXES)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            det.warp(**args)
    # the refusals that existing tests pin stay: no tps model for the inverse paths
    from imm_amd import alignment as AL
    from alignment_reference import jittered_grid_template
    gen = model.image_generator(S, max_batch=4)
    with pytest.raises(NotImplementedError, match='tps map is not inverted'):
        gen.repose(ims, torch.from_numpy(poses), SURFACE_BOXES, template=AL.LandmarkTemplate(jittered_grid_template(10, 8), S), model='tps')


def test_generate_script_warps_photos(m128, tmp_path, capsys):
    from PIL import Image
    from imm_amd.inference import LandmarkDetector
    from imm_amd.utils.config import load_configs
    cfg, model, eng, P, St = m128
    root = str(tmp_path / 'celeba')
    names, pixels = make_celeba_tree(root, n=6)
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, ckpt)
    conf = _write_config(tmp_path, root, str(tmp_path / 'logs'))
    imdir = os.path.join(root, 'Img', 'img_align_celeba_hq')
    rows = [(names[0], 20, 10, 180, 150), (names[2], -10, 30, 120, 170), (names[0], 100, 60, 215, 175), (names[5], 0, 0, 150, 100)]
    boxes = str(tmp_path / 'faces.csv')
    with open(boxes, 'w') as f:
        f.write('file,y0,x0,y1,x1\n' + ''.join('%s,%d,%d,%d,%d\n' % r for r in rows))
    _mu, lm = R.landmarks(10, 4, np.random.RandomState(2))
    np.savez(str(tmp_path / 'lm.npz'), landmarks=lm)
    script = os.path.join(ROOT, 'scripts', 'generate.py')
    common = ['--configs', conf, '--checkpoint', ckpt, '--appearance-dir', imdir, '--boxes', boxes, '--batch-size', '4', '--warp']
    det = LandmarkDetector.from_checkpoint(load_configs([conf]).model, ckpt, image_size=S, max_batch=4, device=DEV)
    photos = [pixels[n] for n in names]
    api_rows = [(names.index(r[0]),) + r[1:] for r in rows]
    for feather in (0.125, 0.0):
        out_dir = str(tmp_path / ('warped%g' % feather))
        _run_script(script, common + ['--landmarks', str(tmp_path / 'lm.npz'), '--feather', str(feather), '--out-dir', out_dir])
        assert '4 faces re-posed in 6 photos' in capsys.readouterr().out
        assert sorted(os.listdir(out_dir)) == [n.replace('.jpg', '.png') for n in names]
        want = det.warp(photos, lm, api_rows, feather=feather)
        for n, w in zip(names, want):
            png = np.asarray(Image.open(os.path.join(out_dir, n.replace('.jpg', '.png'))))
            assert np.array_equal(png, w.cpu().numpy()), n
            assert (n in (names[0], names[2], names[5])) != np.array_equal(png, pixels[n]), n
    with pytest.raises(ValueError, match='--template does not go with it'):
        _run_script(script, common + ['--landmarks', str(tmp_path / 'lm.npz'), '--template', 'none.npz', '--out-dir', str(tmp_path / 'no')])
