"""Keypoints on the MI355X: the box-crop mode of imm_resize_crop_u8 bit for bit against the host composition, the pose head's
keypoint epilogue (mu and maps unchanged, keypoints against a float64 restatement), LandmarkDetector.keypoints() against detect() on
host-cropped tensors, and the scripts end to end on the synthetic CelebA / MAFL tree."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import image_oracle as IO

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dataset_fixtures import make_celeba_tree                        # noqa: E402
from test_detector_gpu import _run_script, _write_config, make_model   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# |keypoints - float64 restatement| in source pixels: f32 accumulation of 2K terms (x <= S = 128, |W| ~ 0.3, sy <= 2.4); measured
# on MI355X at most 3.5e-4 px (K = 64, M = 16, |kp| up to 1170 px), 1.0e-4 at K = 10
KP_BOUND = 1e-3


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


def pack(ops, ims):
    offs, total = [], 0
    for im in ims:
        offs.append(total)
        total += (im.size + 15) & ~15
    buf = np.zeros(total, np.uint8)
    for im, o in zip(ims, offs):
        buf[o:o + im.size] = im.reshape(-1)
    return (ops.to_device_pinned(buf, DEV), ops.to_device_pinned(np.array(offs, np.int64), DEV),
            ops.to_device_pinned(np.array([im.shape[:2] for im in ims], np.int32), DEV))


def photos(sizes, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes]


# ----------------------------------------------------------------------------------------------------------------------------
# 1. box-crop mode
# ----------------------------------------------------------------------------------------------------------------------------
def test_box_crop_mode_bit_exact(ops):
    ims = photos([(218, 178), (90, 200), (300, 250)], 0)
    boxes = [(0, 30, 20, 190, 160),          # inside
             (0, -40, 10, 100, 150),         # past the top
             (0, 150, 10, 260, 150),         # past the bottom
             (1, 10, -60, 80, 90),           # past the left
             (1, 5, 120, 85, 260),           # past the right
             (2, -30, -30, 330, 280),        # past every edge
             (2, 400, 300, 500, 420),        # wholly outside: zeros
             (2, 50, 70, 180, 71),           # one pixel wide
             (0, 100, 80, 101, 140),         # one pixel high
             (2, 0, 0, 300, 250),            # three more boxes on image 2
             (2, 100, 60, 227, 187),
             (2, 7, 9, 20, 11)]
    from imm_amd.keypoints import check_boxes
    rows = check_boxes(boxes, len(ims))
    src, offs, hw = pack(ops, ims)
    S = 64
    for ld in (3, 4):                                       # ld_dst > c: written at channel 1 of a 4-channel stack
        out = torch.full((len(rows), S, S, 4), -7.0, device=DEV)
        dst = torch.empty(len(rows), S, S, 3, device=DEV) if ld == 3 else out[..., 1:]
        ops.resize_crop_u8(src, offs, hw, 3, (S, S), (0, 0), (S, S), dst, boxes=ops.to_device_pinned(rows, DEV))
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        for b, (i, y0, x0, y1, x1) in enumerate(rows):
            ref = IO.resize_bilinear(crop_to_box(ims[i], (y0, x0, y1, x1)), S, S)
            assert np.array_equal(got[b], ref), ('box', b, ld, float(np.abs(got[b] - ref).max()))
        if ld == 4:
            assert bool((out[..., 0] == -7.0).all()), 'channel 0 of the stack was written'
    assert not got[6].any()                                 # the box outside the image
    # resize + central crop of a box (the CelebA geometry applied to a box), and boxes == None is the call of before
    ops.resize_crop_u8(src, offs, hw, 3, (80, 80), (8, 8), (S, S), dst, boxes=ops.to_device_pinned(rows[:4], DEV))
    plain = torch.empty(len(ims), S, S, 3, device=DEV)
    ops.resize_crop_u8(src, offs, hw, 3, (S, S), (0, 0), (S, S), plain)
    whole = torch.empty(len(ims), S, S, 3, device=DEV)
    ops.resize_crop_u8(src, offs, hw, 3, (S, S), (0, 0), (S, S), whole,
                       boxes=ops.to_device_pinned(check_boxes([(0, 0) + im.shape[:2] for im in ims], len(ims)), DEV))
    torch.cuda.synchronize()
    for b in range(4):
        i, y0, x0, y1, x1 = rows[b]
        ref = IO.resize_bilinear(crop_to_box(ims[i], (y0, x0, y1, x1)), 80, 80)[8:8 + S, 8:8 + S]
        assert np.array_equal(dst[b].cpu().numpy(), ref), b
    for i, im in enumerate(ims):
        assert np.array_equal(plain[i].cpu().numpy(), IO.resize_bilinear(im, S, S)), i
    assert torch.equal(whole, plain)
    with pytest.raises(ValueError):
        ops.resize_crop_u8(src, offs, hw, 3, (S, S), (0, 0), (S, S), dst, boxes=ops.to_device_pinned(rows.astype(np.int64), DEV))


# ----------------------------------------------------------------------------------------------------------------------------
# 2. the pose head's keypoint epilogue
# ----------------------------------------------------------------------------------------------------------------------------
def restate(mu, w, b, geom, S):
    """float64 host restatement of the epilogue from the kernel's mu."""
    mu = mu.double().cpu().numpy()
    x = ((mu + 1) / 2 * S).reshape(mu.shape[0], -1)
    kp = x @ w.astype(np.float64) + b.astype(np.float64)
    kp = kp.reshape(mu.shape[0], -1, 2)
    g = geom.astype(np.float64)
    return g[:, None, :2] + kp * g[:, None, 2:]


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('K,M,mode', [(10, 5, 'rot'), (64, 16, 'rot'), (3, 1, 'flat'), (30, 5, 'ankush')])
def test_pose_head_keypoint_epilogue(ops, K, M, mode, dt):
    B, C, s, S = 37, 64, 16, 128
    inv_std, ldh, ldg = 10.0, ops.round_up(K, 4), ops.round_up(K, 8)
    g = torch.Generator().manual_seed(K * 100 + M)
    feat = torch.randn(B, 16, 16, C, generator=g).to(dt).to(DEV)
    w = (torch.randn(1, 1, C, K, generator=g) * 0.3).to(DEV)
    bias = (torch.randn(K, generator=g) * 0.5).to(DEV)
    wt = torch.zeros(ops.round_up(K, 128), C, dtype=dt, device=DEV)
    ops.pack_weights(w, wt, 0, 1, 1, C, K, C, wt.shape[0], C)
    rng = np.random.RandomState(K + M)
    W = (rng.standard_normal((2 * K, 2 * M)) * 0.3).astype(np.float32)
    bb = (rng.standard_normal(2 * M) * 20).astype(np.float32)
    geom = np.stack([rng.uniform(-50, 300, B), rng.uniform(-50, 300, B), rng.uniform(0.01, 2.4, B), rng.uniform(0.01, 2.4, B)],
                    1).astype(np.float32)
    W_d, bb_d, geom_d = (torch.from_numpy(a).to(DEV) for a in (W, bb, geom))      # alive until the launches have run
    outs = []
    for with_kp in (False, True):
        heat = torch.full((B, 16, 16, ldh), -3.0, device=DEV)
        mu = torch.zeros(B, K, 2, device=DEV)
        py, px = torch.zeros(B, 16, K, device=DEV), torch.zeros(B, 16, K, device=DEV)
        gauss = torch.zeros(B, s, s, ldg, dtype=dt, device=DEV)
        kp = torch.full((B, M, 2), float('nan'), device=DEV)
        desc = None
        if with_kp:
            desc = ops.keypoint_desc(W_d, bb_d, geom_d, kp, S)
        ops.pose_head_fwd(feat, C, C, wt, bias, B, 16, 16, K, inv_std, s, heat, ldh, mu, py, px, gauss, ldg, dt, mode, keypoints=desc)
        torch.cuda.synchronize()
        outs.append((heat, mu, py, px, gauss.view(torch.int16), kp))
    for name, a, b in zip(('heat', 'mu', 'py', 'px', 'gauss'), outs[0][:5], outs[1][:5]):
        assert torch.equal(a, b), '%s differs with the keypoint descriptor' % name
    kp = outs[1][5].double().cpu().numpy()
    err = float(np.abs(kp - restate(outs[1][1], W, bb, geom, S)).max())
    print('\nKEYPOINT EPILOGUE K=%d M=%d %s %s: max|kp - f64| %.3g px (|kp| up to %.0f)' % (K, M, mode, dt, err, np.abs(kp).max()))
    assert np.isfinite(kp).all() and err < KP_BOUND


def test_pose_head_keypoint_limits(ops):
    from imm_amd import _lib as L
    B, C, K, dt = 2, 64, 10, torch.bfloat16
    feat = torch.zeros(B, 16, 16, C, dtype=dt, device=DEV)
    wt = torch.zeros(128, C, dtype=dt, device=DEV)
    z = lambda *sh: torch.zeros(*sh, device=DEV)
    args = (feat, C, C, wt, z(K), B, 16, 16, K, 10.0, 16, z(B, 16, 16, 12), 12, z(B, K, 2), z(B, 16, K), z(B, 16, K), None, K, dt)
    desc = ops.keypoint_desc(z(2 * K, 10), z(10), z(B, 4), z(B, 5, 2), 128)
    desc.m = 17
    with pytest.raises(ValueError):
        ops.pose_head_fwd(*args, keypoints=desc)
    with pytest.raises(ValueError):
        ops.keypoint_desc(z(2 * K, 34), z(34), z(B, 4), z(B, 17, 2), 128)
    desc = ops.keypoint_desc(z(2 * K, 10), z(10), z(B, 4), z(B, 5, 2), 0)
    with pytest.raises(L.ImmHipError):
        ops.pose_head_fwd(*args, keypoints=desc)


# ----------------------------------------------------------------------------------------------------------------------------
# 3. LandmarkDetector.keypoints()
# ----------------------------------------------------------------------------------------------------------------------------
def fitted_regressor(K, M=5, S=128, bias=True, seed=0):
    from imm_amd.keypoints import LandmarkRegressor
    rng = np.random.RandomState(seed)
    mu = rng.uniform(-0.8, 0.8, size=(80, K, 2)).astype(np.float32)
    A = rng.standard_normal((2 * K, 2 * M)) * 0.3
    pts = ((mu + 1) / 2.0 * S).reshape(80, -1) @ A + 30.0 + rng.standard_normal((80, 2 * M))
    return LandmarkRegressor.fit({'gauss_yx': mu, 'future_landmarks': pts.reshape(80, M, 2)}, [S, S], bias)


def test_keypoints_against_detect_on_host_crops(ops):
    from imm_amd import keypoints as KP
    from imm_amd.inference import LandmarkDetector
    cfg, model, eng, P, St = make_model(10, 128, 2)
    before = (eng.named_parameters(), eng.named_state())
    det = model.landmark_detector(128, max_batch=8)
    reg = fitted_regressor(10)
    ims = photos([(218, 178), (300, 250), (90, 200)], 5)
    boxes = [(0, 20, 10, 200, 170), (1, -30, 40, 180, 260), (1, 100, 0, 290, 190), (1, 0, 0, 300, 250), (2, 10, 60, 90, 140),
             (0, 150, 100, 260, 200), (2, -20, -20, 110, 220)]
    rows = KP.check_boxes(boxes, len(ims))
    kp, mu = det.keypoints(ims, reg, boxes=boxes, return_mu=True)
    crops = np.stack([IO.resize_bilinear(crop_to_box(ims[i], (y0, x0, y1, x1)), 128, 128) for i, y0, x0, y1, x1 in rows])
    mu_ref = det.detect(torch.from_numpy(crops))
    torch.cuda.synchronize()
    assert kp.shape == (7, 5, 2) and mu.shape == (7, 10, 2)
    assert torch.equal(mu, mu_ref), 'landmarks of the box crops != detect() on the host crops'
    geom = KP.box_geometry(rows, 128)
    host = KP.to_source_pixels(reg.predict(mu_ref.cpu().numpy()), geom)
    err = float(np.abs(kp.double().cpu().numpy() - host).max())
    print('\nKEYPOINTS vs detect() + host predict: max %.3g px' % err)
    assert err < KP_BOUND
    # without boxes: whole images, the same as their whole-image boxes
    whole = det.keypoints(ims, reg)
    assert torch.equal(whole, det.keypoints(ims, reg, boxes=[(0, 0) + im.shape[:2] for im in ims]))
    assert torch.equal(det.keypoints(ims, reg, boxes=[(0, 0) + im.shape[:2] for im in ims], return_mu=True)[1], det.detect(ims))
    # tensor input: the S x S frame, geometry (0, 0, 1, 1)
    kp_t, mu_t = det.keypoints(torch.from_numpy(crops), reg, return_mu=True)
    assert torch.equal(mu_t, mu_ref)
    assert float(np.abs(kp_t.double().cpu().numpy() - reg.predict(mu_t.cpu().numpy())).max()) < KP_BOUND
    with pytest.raises(ValueError):
        det.keypoints(torch.from_numpy(crops), reg, boxes=[(0, 0, 10, 10)] * 7)
    with pytest.raises(ValueError):
        det.keypoints(ims, fitted_regressor(9))
    # a face's result does not depend on its position in the bucket or on its batchmates
    other = photos([(120, 140), (218, 178)], 9)
    perm = [(1, 150, 100, 260, 200), (0, 0, 0, 50, 50), (0, 10, 10, 100, 130), (1, 20, 10, 200, 170), (0, 5, 5, 119, 139)]
    kp2, mu2 = det.keypoints([other[0], ims[0]], reg, boxes=perm, return_mu=True)
    for a, b in ((0, 5), (3, 0)):
        assert torch.equal(kp2[a], kp[b]) and torch.equal(mu2[a], mu[b]), (a, b)
    # captured graphs and plain launches
    det_ng = LandmarkDetector(model, 128, max_batch=8, use_graph=False)
    kp_ng, mu_ng = det_ng.keypoints(ims, reg, boxes=boxes, return_mu=True)
    assert torch.equal(kp_ng, kp) and torch.equal(mu_ng, mu)
    # detect() between keypoints() calls is unchanged, and the model is untouched
    assert torch.equal(det.detect(torch.from_numpy(crops)), mu_ref)
    after = (eng.named_parameters(), eng.named_state())
    for a, b in zip(before, after):
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


# ----------------------------------------------------------------------------------------------------------------------------
# 4. end to end: scripts/test.py --save-regressor, keypoints() on MAFL, scripts/detect.py --regressor --boxes
# ----------------------------------------------------------------------------------------------------------------------------
def test_scripts_end_to_end(ops, tmp_path, capsys):
    from PIL import Image
    from imm_amd.eval import eval_imm
    from imm_amd.inference import LandmarkDetector
    from imm_amd.keypoints import LandmarkRegressor
    from imm_amd.utils.config import load_configs
    from imm_amd.utils.dataset_import import import_dataset
    root = str(tmp_path / 'celeba')
    make_celeba_tree(root, n=40)
    cfg, model, eng, P, St = make_model(3, 128, 4)
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, ckpt)
    conf = _write_config(tmp_path, root, str(tmp_path / 'logs'), n_maps=3)
    regp = str(tmp_path / 'reg.npz')
    printed = []
    for extra in ([], ['--save-regressor', regp]):
        _run_script(os.path.join(ROOT, 'scripts', 'test.py'), ['--configs', conf, '--train-dataset', 'mafl', '--test-dataset', 'mafl',
                                                               '--checkpoint', ckpt, '--batch-size', '4', '--detector'] + extra)
        m = re.search(r'error on mafl datset test set: ([0-9.]+) \(([0-9.]+) percent\)', capsys.readouterr().out)
        assert m is not None
        printed.append(m.group(0))
    assert printed[0] == printed[1], printed
    det = LandmarkDetector.from_checkpoint(load_configs([conf]).model, ckpt, max_batch=4, device=DEV)
    reg = LandmarkRegressor.load(regp, detector=det)
    assert (reg.K, reg.M, reg.S, reg.dataset, reg.checkpoint) == (3, 5, 128, 'mafl', ckpt)
    # the error recomputed from keypoints() on the MAFL test split (its S x S tensors: the frame of its annotations)
    test = import_dataset('celeba')(root, dataset='mafl', subset='test', order_stream=True, tps=False, image_size=[128, 128])
    gt, kps, mus = [], [], []
    for inputs in test.get_dataset(4, repeat=False, shuffle=False, device=DEV):
        kp, mu = det.keypoints(inputs['future_image'], reg, return_mu=True)
        kps.append(kp.cpu().numpy())
        mus.append(mu.cpu().numpy())
        lm = inputs['future_landmarks']
        gt.append(lm.cpu().numpy() if torch.is_tensor(lm) else np.asarray(lm))
    gt, kps, mus = np.concatenate(gt), np.concatenate(kps), np.concatenate(mus)
    err_host = eval_imm.interocular_error(gt, reg.predict(mus))
    err_kp = eval_imm.interocular_error(gt, kps)
    with capsys.disabled():
        print('\nMAFL inter-ocular error: printed %s, host predict %.7f, keypoints() %.7f (rel %.2e)' % (
            printed[0].split(': ')[1], err_host, err_kp, abs(err_kp - err_host) / err_host))
    assert '%.5f' % err_host in printed[0]
    assert abs(err_kp - err_host) <= 1e-5 * err_host
    # scripts/detect.py --regressor --boxes
    imdir = tmp_path / 'faces'
    imdir.mkdir()
    ims = photos([(218, 178), (300, 250), (128, 128)], 3)
    for i, im in enumerate(ims):
        Image.fromarray(im).save(imdir / ('%02d.png' % i))
    rows = [('01.png', 10, 20, 200, 210), ('00.png', -10, 0, 150, 178), ('01.png', 150, 100, 320, 260), ('02.png', 0, 0, 128, 128)]
    with open(str(tmp_path / 'boxes.csv'), 'w') as f:
        f.write('file,y0,x0,y1,x1\n' + ''.join('%s,%d,%d,%d,%d\n' % r for r in rows))
    out = str(tmp_path / 'kp.npz')
    _run_script(os.path.join(ROOT, 'scripts', 'detect.py'), ['--configs', conf, '--checkpoint', ckpt, '--images-dir', str(imdir),
                                                             '--out', out, '--regressor', regp, '--boxes', str(tmp_path / 'boxes.csv'),
                                                             '--plot', str(tmp_path / 'sheet.png'), '--batch-size', '4'])
    assert '4 faces' in capsys.readouterr().out
    r = np.load(out)
    assert r['keypoints'].shape == (4, 5, 2) and r['mu'].shape == (3, 3, 2)
    np.testing.assert_array_equal(r['owner'], [1, 0, 1, 2])
    np.testing.assert_array_equal(r['boxes'], [list(x[1:]) for x in rows])
    ref = det.keypoints(ims, reg, boxes=[(o,) + tuple(b) for o, b in zip(r['owner'], r['boxes'])])
    np.testing.assert_array_equal(r['keypoints'], ref.cpu().numpy())
    assert os.path.exists(str(tmp_path / 'sheet.png'))
