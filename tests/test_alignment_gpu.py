"""Alignment on the MI355X: imm_align_coeffs against the f64 fits, imm_align_warp_u8 against the f64 restatement of the conventions
(tests/alignment_reference.py, every pixel compared), the identity cases (bit for bit), LandmarkDetector.align() against detect() on
host-made crops, its invariances, the program's shape and the scripts end to end on the synthetic CelebA tree."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import image_oracle as IO

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alignment_reference as R                                             # noqa: E402
from dataset_fixtures import make_celeba_tree                                # noqa: E402
from test_detector_gpu import _run_script, _write_config, make_model          # noqa: E402

from imm_amd import alignment as AL                                          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 128
# Largest displacement of T_b over the So x So grid between the kernel's coefficients and the f64 fit of the kernel's own mu, in crop
# pixels at S = 128 (jittered-grid templates, landmark noise sigma 0.08, lam in {0, 1e-3, 0.1}).  Measured on MI355X: see
# COEF_MEASURED; the bound is at most 3x that per K and never above the issue's 0.02 px condition.
COEF_MEASURED = {10: 1.35e-4, 30: 1.0e-3, 50: 4.07e-3, 64: 5.48e-3}
COEF_BOUND = {k: min(3.0 * v, 0.02) for k, v in COEF_MEASURED.items()}
# |aligned - f64 restatement| over every pixel, in grey levels of [0, 255], driven by the kernel's own coef: the f32 rounding of the
# source coordinate times the local gradient of the photo, which is steepest (up to 255 per pixel) at the zero-padded border, where
# every maximum below was found (the mean over all pixels is 1e-5).  The coordinate (up to ~300 px) is rounded to ~1e-5 px by the
# affine part alone (m3 = 3); the tps map adds an f32 sum of K terms U(|q - t_j|^2) coef_j over an f32 basis, whose rounding is
# 2^-24 sum_j |U_j coef_j| * S / 2 * sy: ~1e-3 px at K = 64.  Measured on MI355X per m3 (So in {64, 128, 160}; landmarks = the
# template rotated, scaled, shifted and jittered with sigma 0.04): WARP_MEASURED; the bound is 3x that.
WARP_MEASURED = {3: 6.49e-3, 13: 4.75e-3, 53: 0.108, 67: 0.225}


def warp_bound(m3):
    return 3.0 * WARP_MEASURED[min(k for k in WARP_MEASURED if k >= m3)]


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


def crop_to_box(image, box):
    from imm_amd.datasets.impair_dataset import ImagePairDataset
    return ImagePairDataset._crop_to_box(None, image, box, pad=True)


def dev(ops, a, dtype=None):
    return ops.to_device_pinned(np.ascontiguousarray(a), DEV, dtype)


def gpu_coeffs(ops, tpl, mu32, model, lam=0.0):
    """imm_align_coeffs on f32 landmarks [n, K, 2] -> f32 [n, m3, 2] (host array)."""
    K, m3 = tpl.K, AL.n_basis(model, tpl.K)
    ft = dev(ops, tpl.fit_matrix(model, lam).T.astype(np.float32))
    mu_d = dev(ops, mu32)
    coef = torch.full((len(mu32), m3, 2), float('nan'), device=DEV)
    ops.align_coeffs(mu_d, ft, K, m3, coef)
    torch.cuda.synchronize()
    return coef.cpu().numpy()


def displacement_px(t, coef_a, coef_b, So=S):
    """max over the So x So grid of |T_a(q) - T_b(q)| in crop pixels at S = 128."""
    basis = R.basis_at(t, R.grid(So), np.shape(coef_a)[-2] > 3)
    d = basis.T @ (np.asarray(coef_a, np.float64) - np.asarray(coef_b, np.float64))
    return float(np.abs(d).max()) * S / 2.0


CASES = [('similarity', 0.0), ('affine', 0.0), ('tps', 0.0), ('tps', 1e-3), ('tps', 0.1)]


# ----------------------------------------------------------------------------------------------------------------------------
# 1. coefficients
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [10, 30, 50, 64])
def test_align_coeffs_against_f64(ops, K):
    t = R.jittered_grid_template(K, K)
    tpl = AL.LandmarkTemplate(t, S)
    rng = np.random.RandomState(K + 1)
    mu32 = (t[None] + rng.standard_normal((37, K, 2)) * 0.08).astype(np.float32)
    worst = 0.0
    for model, lam in CASES:
        coef = gpu_coeffs(ops, tpl, mu32, model, lam)
        assert np.isfinite(coef).all()
        err = max(displacement_px(t, coef[b], R.fit(t, mu32[b].astype(np.float64), model, lam)) for b in range(len(mu32)))
        print('\nALIGN COEFFS K=%d %s lam=%g: max displacement %.3g px' % (K, model, lam, err))
        worst = max(worst, err)
    print('ALIGN COEFFS K=%d worst %.3g px (bound %.3g)' % (K, worst, COEF_BOUND[K]))
    assert worst <= COEF_BOUND[K]


def test_align_coeffs_limits(ops):
    from imm_amd import _lib as L
    z = lambda *sh: torch.zeros(*sh, device=DEV)
    with pytest.raises(ValueError):
        ops.align_coeffs(z(2, 10, 2), z(20, 7), 10, 3, z(2, 3, 2))
    with pytest.raises(L.ImmHipError):
        ops.align_coeffs(z(2, 65, 2), z(130, 136), 65, 68, z(2, 68, 2))
    with pytest.raises(ValueError):                                  # tps needs the basis, m3 = 3 takes none
        ops.align_warp_u8(z(2, S, S, 3), None, None, None, z(2, 4), z(2, 13, 2), None, S, z(2, 64, 64, 3))
    with pytest.raises(ValueError):
        ops.align_warp_u8(z(2, S, S, 3), None, None, None, z(2, 4), z(2, 3, 2), z(3, 64 * 64), S, z(2, 64, 64, 3))


# ----------------------------------------------------------------------------------------------------------------------------
# 2. the warp
# ----------------------------------------------------------------------------------------------------------------------------
def pack(ops, ims):
    offs, total = [], 0
    for im in ims:
        offs.append(total)
        total += (im.size + 15) & ~15
    buf = np.zeros(max(total, 16), np.uint8)
    for im, o in zip(ims, offs):
        buf[o:o + im.size] = im.reshape(-1)
    return dev(ops, buf), dev(ops, np.array(offs, np.int64)), dev(ops, np.array([im.shape[:2] for im in ims], np.int32))


PHOTOS = [(218, 178), (96, 300), (31, 47)]
BOXES = [(0, 30, 20, 190, 160), (0, -40, 10, 100, 150), (0, 150, 10, 260, 150), (0, 0, 0, 218, 178),
         (1, 10, -60, 80, 90), (1, 5, 120, 85, 260), (1, -30, -30, 130, 330), (1, 300, 400, 400, 520),     # the last: wholly outside
         (2, 0, 0, 31, 47), (2, -10, -10, 40, 60), (2, 5, 7, 20, 30)]


def run_warp(ops, ims, rows, tpl, coef32, So, model):
    from imm_amd import keypoints as KP
    src, offs, hw = pack(ops, ims)
    geom = KP.box_geometry(rows, S)
    basis = dev(ops, tpl.basis('tps', So).astype(np.float32)) if model == 'tps' else None
    out = torch.full((len(rows), So, So, 3), float('nan'), device=DEV)
    ops.align_warp_u8(src, offs, hw, dev(ops, rows), dev(ops, geom), dev(ops, coef32), basis, S, out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), geom


@pytest.mark.parametrize('So', [64, 128, 160])
@pytest.mark.parametrize('model', ['similarity', 'affine', 'tps'])
@pytest.mark.parametrize('K', [10, 50, 64])
def test_align_warp_against_f64(ops, K, model, So):
    from imm_amd import keypoints as KP
    ims = [R.smooth_photo(h, w, 10 + i) for i, (h, w) in enumerate(PHOTOS)]
    rows = KP.check_boxes(BOXES, len(ims))
    t = R.jittered_grid_template(K, 3)
    tpl = AL.LandmarkTemplate(t, S)
    rng = np.random.RandomState(So)
    # landmarks: the template rotated, scaled and shifted per row, plus noise (the maps then leave the boxes here and there)
    mu = []
    for _ in rows:
        th, s = rng.uniform(-0.5, 0.5), rng.uniform(0.6, 1.2)
        rot = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        mu.append(t @ rot.T + rng.uniform(-0.2, 0.2, 2) + rng.standard_normal(t.shape) * 0.04)
    coef = gpu_coeffs(ops, tpl, np.stack(mu).astype(np.float32), model)
    got, geom = run_warp(ops, ims, rows, tpl, coef, So, model)
    ref = R.warp(ims, rows[:, 0], geom, coef, t, S, So)
    assert got.shape == ref.shape == (len(rows), So, So, 3) and np.isfinite(got).all()
    err = np.abs(got - ref)                                        # every pixel of every row
    print('\nALIGN WARP K=%d %s So=%d: max |gpu - f64| %.3g grey levels (mean %.3g)' % (K, model, So, err.max(), err.mean()))
    assert err.max() <= warp_bound(coef.shape[1])
    outside = R.wholly_outside(ims, rows[:, 0], geom, coef, t, S, So)
    assert outside[7].all() and outside.sum() > outside[7].sum()    # the far box, and corners of others
    assert not got[outside].any(), 'a pixel whose four taps lie outside the photo is not exactly 0'
    assert got.min() >= 0.0 and got.max() <= 255.0


# ----------------------------------------------------------------------------------------------------------------------------
# 3. identity
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [10, 30, 64])
def test_own_landmarks_give_the_identity_map(ops, K):
    rng = np.random.RandomState(K)
    worst = 0.0
    for r in range(3):
        mu32 = (R.jittered_grid_template(K, 40 + r) + rng.standard_normal((K, 2)) * 0.02).astype(np.float32)
        tpl = AL.LandmarkTemplate(mu32.astype(np.float64), S)
        for model in AL.MODELS:
            coef = gpu_coeffs(ops, tpl, mu32[None], model)[0]
            ident = np.zeros_like(coef, dtype=np.float64)
            ident[-2, 0] = ident[-1, 1] = 1.0
            worst = max(worst, displacement_px(tpl.points, coef, ident))
    print('\nALIGN IDENTITY K=%d: max displacement from the identity %.3g px (bound %.3g)' % (K, worst, COEF_BOUND[K]))
    assert worst <= COEF_BOUND[K]


@pytest.mark.parametrize('model', ['affine', 'tps'])
def test_identity_warp_is_bit_exact(ops, model):
    from imm_amd import keypoints as KP
    rng = np.random.RandomState(2)
    ims = [rng.randint(0, 256, size=(S, S, 3)).astype(np.uint8) for _ in range(3)]
    rows = KP.check_boxes([(0, 0, S, S)] * 3, 3)
    t = R.jittered_grid_template(10, 6)
    tpl = AL.LandmarkTemplate(t, S)
    m3 = AL.n_basis(model, 10)
    coef = np.zeros((3, m3, 2), np.float32)
    coef[:, -2, 0] = coef[:, -1, 1] = 1.0
    got, geom = run_warp(ops, ims, rows, tpl, coef, S, model)
    assert np.array_equal(geom, np.tile(np.array([0, 0, 1, 1], np.float32), (3, 1)))
    assert np.array_equal(got, np.stack(ims).astype(np.float32)), 'the identity warp is not the photo bit for bit'
    # the f32 source mode (a tensor batch is its own source)
    src = torch.from_numpy(np.stack(ims).astype(np.float32)).to(DEV) + 0.25
    out = torch.full((3, S, S, 3), float('nan'), device=DEV)
    basis = dev(ops, tpl.basis('tps', S).astype(np.float32)) if model == 'tps' else None
    ops.align_warp_u8(src, None, None, None, dev(ops, geom), dev(ops, coef), basis, S, out)
    torch.cuda.synchronize()
    assert torch.equal(out, src)


# ----------------------------------------------------------------------------------------------------------------------------
# 4. LandmarkDetector.align()
# ----------------------------------------------------------------------------------------------------------------------------
def photos(sizes, seed):
    return [R.smooth_photo(h, w, seed + i) for i, (h, w) in enumerate(sizes)]


FACE_BOXES = [(0, 20, 10, 200, 170), (1, -30, 40, 180, 260), (1, 100, 0, 290, 190), (1, 0, 0, 300, 250), (2, 10, 60, 90, 140),
              (0, 150, 100, 260, 200), (2, -20, -20, 110, 220)]


@pytest.mark.parametrize('K', [10, 50])
def test_align_against_detect_on_host_crops(ops, K):
    from imm_amd import keypoints as KP
    cfg, model, eng, P, St = make_model(K, S, 2)
    det = model.landmark_detector(S, max_batch=8)
    ims = photos([(218, 178), (300, 250), (90, 200)], 5)
    rows = KP.check_boxes(FACE_BOXES, len(ims))
    geom = KP.box_geometry(rows, S)
    crops = np.stack([IO.resize_bilinear(crop_to_box(ims[i], (y0, x0, y1, x1)), S, S) for i, y0, x0, y1, x1 in rows])
    mu_ref = det.detect(torch.from_numpy(crops))
    torch.cuda.synchronize()
    mu64 = mu_ref.double().cpu().numpy()
    # a well-separated template (cond(L) <= 2e3).  The mean shape of THIS model's landmarks would not do: an untrained model puts
    # all K of them within a few hundredths of each other, L is then next to singular and a spline between such clouds folds over
    # itself (measured with that template at K = 50: coefficients 0.3 px and image 58 grey levels off) - garbage in, not alignment.
    t = R.jittered_grid_template(K, K + 5)
    tpl = AL.LandmarkTemplate(t, S)
    for kind, lam, So in (('similarity', 0.0, S), ('affine', 0.0, 96), ('tps', 0.0, S), ('tps', 0.1, 160)):
        img, al = det.align(ims, tpl, boxes=FACE_BOXES, model=kind, lam=lam, out_size=So, return_transform=True)
        torch.cuda.synchronize()
        assert img.shape == (7, So, So, 3) and img.dtype == torch.float32 and img.device.type == 'cuda'
        assert torch.equal(al.mu, mu_ref), 'landmarks of the box crops != detect() on the host crops'
        assert np.array_equal(al.geom.cpu().numpy(), geom) and (al.model, al.lam, al.out_size) == (kind, lam, So)
        coef = al.coef.cpu().numpy()
        assert coef.shape == (7, AL.n_basis(kind, K), 2)
        cerr = max(displacement_px(t, coef[b], R.fit(t, mu64[b], kind, lam), So) for b in range(7))
        ref = R.warp(ims, rows[:, 0], geom, coef, t, S, So)
        werr = float(np.abs(img.cpu().numpy() - ref).max())
        print('\nALIGN() K=%d %s lam=%g So=%d: coefficients %.3g px off the host fit, image %.3g grey levels off the restatement' % (
            K, kind, lam, So, cerr, werr))
        assert cerr <= COEF_BOUND[K] and werr <= warp_bound(coef.shape[1])
        # the Alignment object's point map is the one the pixels were sampled through
        src_pts = al.to_source(np.array([[0.0, 0.0], [So / 2.0, So / 3.0]]))
        c = (R.apply_map(t, coef[2], -1 + 2 * np.array([[0.0, 0.0], [So / 2.0, So / 3.0]]) / So) + 1) / 2 * S
        assert np.abs(src_pts[2] - (geom[2, :2] + c * geom[2, 2:])).max() < 1e-9
    # So == S: the aligned batch feeds detect() without leaving the GPU
    img = det.align(ims, tpl, boxes=FACE_BOXES)
    assert det.detect(img).shape == (7, K, 2)
    # without boxes: whole photos, the same as their whole-photo boxes
    assert torch.equal(det.align(ims, tpl), det.align(ims, tpl, boxes=[(0, 0) + im.shape[:2] for im in ims]))
    assert torch.equal(det.landmarks(ims, boxes=FACE_BOXES), mu_ref)
    with pytest.raises(ValueError):
        det.align(ims, AL.LandmarkTemplate(R.jittered_grid_template(K + 1, 1), S))
    with pytest.raises(ValueError):
        det.align(ims, tpl, model='affine', lam=0.5)
    with pytest.raises(ValueError):
        det.align(torch.from_numpy(crops), tpl, boxes=[(0, 0, 10, 10)] * 7)


def test_align_tensor_batch_is_its_own_source(ops):
    cfg, model, eng, P, St = make_model(10, S, 2)
    det = model.landmark_detector(S, max_batch=4)
    g = torch.Generator().manual_seed(3)
    # smooth f32 crops (not u8-valued), more than one bucket
    base = np.stack([R.smooth_photo(S, S, 50 + i).astype(np.float32) for i in range(6)])
    crops = torch.from_numpy(base) * 0.9 + torch.rand(6, 1, 1, 3, generator=g)
    tpl = AL.LandmarkTemplate(R.jittered_grid_template(10, 2), S)
    for kind in ('similarity', 'tps'):
        img, al = det.align(crops, tpl, model=kind, out_size=64, return_transform=True)
        torch.cuda.synchronize()
        assert torch.equal(al.mu, det.detect(crops))
        geom = al.geom.cpu().numpy()
        assert np.array_equal(geom, np.tile(np.array([0, 0, 1, 1], np.float32), (6, 1)))
        ref = R.warp(list(crops.numpy()), np.arange(6), geom, al.coef.cpu().numpy(), tpl.points, S, 64)
        err = float(np.abs(img.cpu().numpy() - ref).max())
        print('\nALIGN() tensor batch %s: %.3g grey levels off the restatement' % (kind, err))
        assert err <= warp_bound(al.coef.shape[1])
        assert torch.equal(img, det.align(crops.to(DEV), tpl, model=kind, out_size=64))      # a device tensor is read the same way


def test_align_invariances(ops):
    from imm_amd.inference import LandmarkDetector
    from imm_amd.keypoints import LandmarkRegressor
    cfg, model, eng, P, St = make_model(10, S, 2)
    before = (eng.named_parameters(), eng.named_state())
    det = model.landmark_detector(S, max_batch=8)
    ims = photos([(218, 178), (300, 250), (90, 200)], 5)
    tpl = AL.LandmarkTemplate(R.jittered_grid_template(10, 8), S)
    rng = np.random.RandomState(0)
    reg = LandmarkRegressor(rng.standard_normal((10, 20)) * 0.3, rng.standard_normal(10) * 5, 10, S, True)
    crops = torch.from_numpy(np.stack([IO.resize_bilinear(im, S, S) for im in ims]))
    mu0, kp0 = det.detect(crops), det.keypoints(ims, reg, boxes=FACE_BOXES)
    mu0_u8 = det.detect(ims)
    for kind in AL.MODELS:
        img, al = det.align(ims, tpl, boxes=FACE_BOXES, model=kind, return_transform=True)
        # a row's result does not depend on its position in the bucket or on its batchmates (other buckets, other photos around it)
        other = photos([(120, 140)], 9)
        perm = [(1, 150, 100, 260, 200), (0, 0, 0, 50, 50), (0, 10, 10, 100, 130), (1, 20, 10, 200, 170), (0, 5, 5, 119, 139)]
        img2, al2 = det.align([other[0], ims[0]], tpl, boxes=perm, model=kind, return_transform=True)
        for a, b in ((0, 5), (3, 0)):
            assert torch.equal(img2[a], img[b]) and torch.equal(al2.coef[a], al.coef[b]), (kind, a, b)
        # several buckets of the same size: 16 rows through two buckets of 8 (across bucket SIZES detect() itself moves by a few
        # 1e-6: tests/test_detector_gpu.py test_batch_independence_and_repeatability)
        many = det.align(ims, tpl, boxes=FACE_BOXES + FACE_BOXES + FACE_BOXES[:2], model=kind)
        assert torch.equal(many[:7], img) and torch.equal(many[7:14], img) and torch.equal(many[14:], img[:2])
        # two boxes on one photo == the same boxes on two copies of the photo
        two = det.align([ims[1]], tpl, boxes=[(0, -30, 40, 180, 260), (0, 100, 0, 290, 190)], model=kind)
        copies = det.align([ims[1], ims[1].copy()], tpl, boxes=[(0, -30, 40, 180, 260), (1, 100, 0, 290, 190)], model=kind)
        assert torch.equal(two, copies)
        # captured graphs and plain launches, and a repeat
        det_ng = LandmarkDetector(model, S, max_batch=8, use_graph=False)
        assert torch.equal(det_ng.align(ims, tpl, boxes=FACE_BOXES, model=kind), img)
        assert torch.equal(det.align(ims, tpl, boxes=FACE_BOXES, model=kind), img)
        # detect() and keypoints() between align() calls are unchanged
        assert torch.equal(det.detect(crops), mu0) and torch.equal(det.detect(ims), mu0_u8)
        assert torch.equal(det.keypoints(ims, reg, boxes=FACE_BOXES), kp0)
    after = (eng.named_parameters(), eng.named_state())
    for a, b in zip(before, after):
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_align_program_shape(ops):
    cfg, model, eng, P, St = make_model(10, S, 2)
    det = model.landmark_detector(S, max_batch=8)
    base = det.program(8, u8=True)
    for kind in AL.MODELS:
        prog = det.program(8, u8=True, align=(kind, AL.n_basis(kind, 10)))
        assert len(prog) - len(base) <= 2
        assert [(l.tag, l.family) for l in prog[:len(base)]] == [(l.tag, l.family) for l in base]
        assert [l.tag for l in prog[len(base):]] == ['align_coeffs', 'align_warp']
    assert [l.tag for l in det.program(8)] == [l.tag for l in base[1:]]
    with pytest.raises(ValueError):
        det.program(8, align=('tps', 3))
    with pytest.raises(ValueError):
        det.program(8, kp_m=5, align=('affine', 3))
    ims = photos([(218, 178), (90, 200)], 1)
    tpl = AL.LandmarkTemplate(R.jittered_grid_template(10, 8), S)
    det.align(ims, tpl, model='similarity')
    det.align(ims, tpl, model='affine', out_size=64)
    assert det._al_basis == {}, 'similarity / affine allocated a basis buffer'
    det.align(ims, tpl, model='tps')
    det.align(ims, tpl, model='tps', lam=0.1)
    assert len(det._al_basis) == 1 and list(det._al_basis.values())[0].shape == (13, S * S)


# ----------------------------------------------------------------------------------------------------------------------------
# 5. the scripts
# ----------------------------------------------------------------------------------------------------------------------------
def test_align_scripts_end_to_end(ops, tmp_path, capsys):
    from PIL import Image
    root = str(tmp_path / 'celeba')
    make_celeba_tree(root, n=40)
    cfg, model, eng, P, St = make_model(3, S, 4)
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, ckpt)
    conf = _write_config(tmp_path, root, str(tmp_path / 'logs'), n_maps=3)
    # scripts/test.py --save-template: a loadable template of the training split's mean shape
    tplp = str(tmp_path / 'mafl_template.npz')
    _run_script(os.path.join(ROOT, 'scripts', 'test.py'), ['--configs', conf, '--train-dataset', 'mafl', '--test-dataset', 'mafl',
                                                           '--checkpoint', ckpt, '--batch-size', '4', '--detector', '--save-template', tplp])
    assert 'error on mafl datset test set' in capsys.readouterr().out
    saved = AL.LandmarkTemplate.load(tplp)
    assert (saved.K, saved.S, saved.dataset, saved.checkpoint) == (3, S, 'mafl', ckpt)
    # scripts/align.py --fit-template, then --template, on the tree's photos
    imdir = os.path.join(root, 'Img', 'img_align_celeba_hq')
    files = sorted(os.listdir(imdir))
    ims = [np.asarray(Image.open(os.path.join(imdir, f)).convert('RGB')) for f in files]
    h, w = ims[0].shape[:2]
    rows = [(files[3], 10, 5, h - 10, w - 5), (files[0], -10, 0, h // 2 + 40, w), (files[3], 0, 0, h, w), (files[7], 20, 10, h, w + 15)]
    boxes = str(tmp_path / 'boxes.csv')
    with open(boxes, 'w') as f:
        f.write('file,y0,x0,y1,x1\n' + ''.join('%s,%d,%d,%d,%d\n' % r for r in rows))
    fitted = str(tmp_path / 'fitted.npz')
    common = ['--configs', conf, '--checkpoint', ckpt, '--images-dir', imdir, '--boxes', boxes, '--batch-size', '4']
    results = []
    for k, (extra, kind, So) in enumerate(((['--fit-template', fitted], 'similarity', 128), (['--template', fitted], 'tps', 64))):
        out_dir, npz = str(tmp_path / ('aligned%d' % k)), str(tmp_path / ('aligned%d.npz' % k))
        _run_script(os.path.join(ROOT, 'scripts', 'align.py'), common + extra + ['--model', kind, '--out-size', str(So), '--out-dir', out_dir,
                                                                                 '--npz', npz])
        assert '4 faces aligned' in capsys.readouterr().out
        r = np.load(npz)
        pngs = sorted(os.listdir(out_dir))
        assert len(pngs) == 4
        tpl = AL.LandmarkTemplate.load(fitted)
        assert np.array_equal(r['template'], tpl.points) and str(r['model']) == kind and int(r['out_size']) == So
        assert r['coef'].shape == (4, AL.n_basis(kind, 3), 2) and r['mu'].shape == (4, 3, 2)
        np.testing.assert_array_equal(r['owner'], [3, 0, 3, 7])
        np.testing.assert_array_equal(r['boxes'], [list(x[1:]) for x in rows])
        ref = R.warp(ims, r['owner'], r['geom'], r['coef'], tpl.points, S, So)
        for b, name in enumerate(pngs):
            assert name.startswith('%04d_' % b)
            png = np.asarray(Image.open(os.path.join(out_dir, name))).astype(np.float64)
            assert png.shape == (So, So, 3)
            assert np.abs(png - np.clip(ref[b], 0, 255)).max() <= 0.5 + warp_bound(r['coef'].shape[1]), (kind, name)
        results.append(r)
    # the fitted template is the refined mean shape of these four faces' landmarks
    want = AL.LandmarkTemplate.from_landmarks(results[0]['mu'], S)
    assert np.array_equal(want.points, AL.LandmarkTemplate.load(fitted).points)
    np.testing.assert_array_equal(results[0]['mu'], results[1]['mu'])
