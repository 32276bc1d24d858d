"""Face tracking on the MI355X: imm_track_step in guarded buffers against the numpy restatement of include/imm_track.h
(tests/track_reference.py) bit for bit, LandmarkDetector.track against the loop over public calls it replaces (landmarks() per frame,
the restatement, the next frame's boxes on the host), the equalities between track(), its chunks and the live tracker, and the script.

"Bit for bit" compares the stored bits of every element; two NaNs count as equal whatever their payloads, which IEEE 754 leaves
to the implementation (a NaN landmark is an input of these cases)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alignment_reference as AR                  # noqa: E402
import guarded                                    # noqa: E402
import test_detector_gpu as D                     # noqa: E402  (make_model, _run_script, _write_config)
import track_reference as R                       # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OE = (1.0, 0.05, 1.0)
FPS = 25.0


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


@pytest.fixture(autouse=True)
def _guards_intact():
    guarded.reset()
    yield
    guarded.check_guards()


def same_bits(got, ref, what):
    """Every element's stored bits equal; NaN matches NaN."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref = np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if got.dtype.kind == 'f':
        view = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), '%s: NaNs at other places' % what
        bad = (got.view(view) != ref.view(view)) & ~nan
    else:
        bad = got != ref
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError('%s: %d of %d elements differ, first at %s: got %r, want %r' % (what, int(bad.sum()), bad.size, i, got[i], ref[i]))


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the restatement
# ----------------------------------------------------------------------------------------------------------------------------
def kernel_case(F, K, seed):
    """Four frames of F faces: rectangular boxes (h != w) on three photos (one face names a photo that does not exist), a random
    shape per face that drifts, turns and grows from frame to frame, and the special faces: a NaN / an inf landmark (lost for a
    frame, or from the start), coincident landmarks at the start (den == 0), landmarks a billion boxes wide (the clamps)."""
    rng = np.random.RandomState(seed)
    hw = np.array([[300, 400], [240, 200], [500, 350]], dtype=np.int32)
    h = rng.randint(20, 300, F)
    w = h + rng.choice([-1, 1], F) * rng.randint(3, 15, F)
    y0, x0 = rng.randint(-30, 250, F), rng.randint(-30, 250, F)
    boxes = np.stack([rng.randint(0, 3, F), y0, x0, y0 + h, x0 + w], axis=1).astype(np.int32)
    shape = rng.uniform(-0.8, 0.8, size=(F, K, 2))
    mus = []
    for t in range(4):
        ang, sc, sh = rng.uniform(-0.2, 0.2, F), rng.uniform(0.85, 1.2, F), rng.uniform(-0.15, 0.15, (F, 1, 2))
        rot = np.stack([np.stack([np.cos(ang), -np.sin(ang)], 1), np.stack([np.sin(ang), np.cos(ang)], 1)], 1) * sc[:, None, None]
        mus.append((np.einsum('fab,fkb->fka', rot, shape) + sh + rng.standard_normal((F, K, 2)) * 0.01).astype(np.float32))
    mus[2][0, K // 2, 1] = np.nan                                   # face 0: lost on frame 2, back on frame 3
    if F >= 3:
        boxes[1, 0] = 7                                             # a photo that does not exist: flagged, never read
        mus[1][2] = ((shape[2] * 1e9) + 1e10).astype(np.float32)    # the clamps, through the measurement
    if F >= 65:
        mus[0][5] = mus[0][5][:1]                                   # coincident at the start: den == 0, lost for good
        mus[0][6, 1, 0] = np.inf                                    # non-finite at the start: the anchor holds it, lost for good
        mus[1][7, 0, 0] = -np.inf
        mus[3][64] = np.float32(0.25)                               # the face of the second block: coincident on the last frame
    return hw, boxes, mus


@pytest.mark.parametrize('K', [3, 10, 64])
@pytest.mark.parametrize('F', [1, 3, 65])
def test_track_step_equals_the_restatement(ops, F, K):
    from imm_amd import keypoints as KP
    S = 128
    hw, boxes, mus = kernel_case(F, K, 100 * F + K)
    one_euro = None if K == 10 else OE                               # K = 10 runs with the filter off
    mc, be, dc = OE
    c, te = 2.0 * np.pi / FPS, 1.0 / FPS
    beta = 0.5
    st_ref = R.new_state(F, K)
    st = guarded.out((F, R.state_size(K)), torch.float64, DEV, fill=0.0)
    hw_d = guarded.inp(torch.from_numpy(hw), DEV)
    rows = boxes
    seen = np.zeros(F, dtype=np.int32)
    for t in range(4):
        next_image = (t + 1) % 3                                     # never the current rows' image index throughout
        mu_d = guarded.inp(torch.from_numpy(mus[t]), DEV)
        rows_d = guarded.inp(torch.from_numpy(rows), DEV)
        pts = guarded.out((F, K, 2), torch.float32, DEV)
        smooth = guarded.out((F, K, 2), torch.float32, DEV)
        nxt = guarded.out((F, 5), torch.int32, DEV)
        geom = guarded.out((F, 4), torch.float32, DEV)
        flags = guarded.out((F,), torch.int32, DEV)
        ops.track_step(mu_d, rows_d, hw_d, st, S, next_image, int(t == 0), beta, mc, be, dc, c, te, one_euro is None, pts, smooth, nxt,
                       geom, flags)
        torch.cuda.synchronize()
        r_pts, r_smooth, r_rows, r_geom, r_flags = R.track_step(mus[t], rows, hw, st_ref, S, next_image, int(t == 0), beta, one_euro, FPS)
        what = 'F=%d K=%d frame %d ' % (F, K, t)
        same_bits(pts, r_pts, what + 'points')
        same_bits(smooth, r_smooth, what + 'points_smooth')
        same_bits(nxt, r_rows, what + 'boxes_next')
        same_bits(geom, r_geom, what + 'geom_next')
        same_bits(flags, r_flags, what + 'flags')
        same_bits(st, st_ref, what + 'state')
        assert np.array_equal(r_geom, KP.box_geometry(r_rows, S)), 'geom_next is box_geometry of the next rows'
        assert (r_rows[:, 0] == next_image).all() and (r_rows[:, 3] > r_rows[:, 1]).all() and (r_rows[:, 4] > r_rows[:, 2]).all()
        assert np.abs(r_rows[:, 1:].astype(np.int64)).max() < 2 ** 24
        rows = r_rows
        seen |= r_flags
        if t == 2:
            assert r_flags[0] & 1, 'the NaN landmark loses face 0 on frame 2'
        if t == 3:
            assert not r_flags[0] & 1, 'and frame 3 finds it again'
    # the case holds what it says it holds
    assert seen[0] & 1
    if F >= 3:
        assert seen[1] & 2 and seen[2] & 2 and (rows[2, 3] - rows[2, 1] > 2 ** 20 or st_ref[2, 4] > 1e3)
    if F >= 65:
        assert seen[5] & 1 and seen[6] & 1 and seen[7] & 1 and seen[64] & 1 and not (seen[8:64] & 1).any()


def test_track_step_may_write_the_rows_it_read(ops):
    """boxes_next may be the buffer `boxes`: a thread reads its row before it writes it."""
    S, F, K = 128, 65, 5
    hw, boxes, mus = kernel_case(F, K, 9)
    st_ref = R.new_state(F, K)
    st = guarded.out((F, R.state_size(K)), torch.float64, DEV, fill=0.0)
    hw_d = guarded.inp(torch.from_numpy(hw), DEV)
    rows_d = guarded.inp(torch.from_numpy(boxes), DEV)
    rows = boxes
    for t in range(3):
        mu_d = guarded.inp(torch.from_numpy(mus[t]), DEV)
        pts, smooth = guarded.out((F, K, 2), torch.float32, DEV), guarded.out((F, K, 2), torch.float32, DEV)
        geom, flags = guarded.out((F, 4), torch.float32, DEV), guarded.out((F,), torch.int32, DEV)
        ops.track_step(mu_d, rows_d, hw_d, st, S, 1, int(t == 0), 1.0, 1.0, 0.05, 1.0, 2.0 * np.pi / FPS, 1.0 / FPS, False, pts, smooth,
                       rows_d, geom, flags)
        torch.cuda.synchronize()
        r = R.track_step(mus[t], rows, hw, st_ref, S, 1, int(t == 0), 1.0, OE, FPS)
        rows = r[2]
        same_bits(rows_d, rows, 'frame %d rows in place' % t)
        same_bits(smooth, r[1], 'frame %d points_smooth' % t)
        same_bits(st, st_ref, 'frame %d state' % t)


# ----------------------------------------------------------------------------------------------------------------------------
# 2. track() against the loop over public calls
# ----------------------------------------------------------------------------------------------------------------------------
T = 5
FACES = [(0, 10, 8, 70, 60), (0, 30, 20, 90, 75), (0, -10, -6, 50, 40)]           # the third reaches outside the photo
FOURTH = (0, 20, 30, 80, 70)
BETA = 0.5


def clip():
    """Five frames of two sizes cut from one smooth photo, each shifted a few pixels from the last."""
    big = AR.smooth_photo(150, 130, 3)
    frames = []
    for t in range(T):
        h, w = ((96, 80), (120, 100))[t % 2]
        oy, ox = 4 + 3 * t, 20 - 2 * t
        frames.append(np.ascontiguousarray(big[oy:oy + h, ox:ox + w]))
    return frames


def fitted_regressor(K, S):
    from imm_amd.keypoints import LandmarkRegressor
    rng = np.random.RandomState(4)
    mu = rng.uniform(-0.8, 0.8, size=(60, K, 2))
    target = (mu[:, :5] + 1.0) * (S / 2.0) + rng.standard_normal((60, 5, 2))
    return LandmarkRegressor.fit({'gauss_yx': mu, 'future_landmarks': target}, [S, S], True)


@pytest.fixture(scope='module')
def world(ops):
    """One model and detector (K = 10, S = 128, max_batch 4), the clip, and the user's loop at the parent commit run once:
    landmarks() (and keypoints()) per frame, the restatement on the host, the next frame's boxes."""
    cfg, model, eng, P, St = D.make_model(10, 128, 2)
    det = model.landmark_detector(128, max_batch=4)
    frames = clip()
    reg = fitted_regressor(10, 128)
    F, K = len(FACES), det.K
    st = R.new_state(F, K)
    rows = np.array(FACES, dtype=np.int32)
    ref = {k: [] for k in ('mu', 'points', 'points_smooth', 'boxes', 'flags', 'keypoints')}
    for t in range(T):
        mu = det.landmarks([frames[t]], rows.tolist()).cpu().numpy()
        kp, mu_kp = det.keypoints([frames[t]], reg, boxes=rows.tolist(), return_mu=True)
        assert np.array_equal(mu_kp.cpu().numpy(), mu)
        pts, smooth, nxt, _geom, flags = R.track_step(mu, rows, [frames[t].shape[:2]], st, det.S, 0, int(t == 0), BETA, OE, FPS)
        for k, v in (('mu', mu), ('points', pts), ('points_smooth', smooth), ('boxes', rows[:, 1:].copy()), ('flags', flags),
                     ('keypoints', kp.cpu().numpy())):
            ref[k].append(v)
        rows = nxt
    return det, frames, reg, {k: np.stack(v) for k, v in ref.items()}


def same_track(tr, ref, what, faces=slice(None), keypoints=False):
    tr = tr.cpu()
    for k in ('mu', 'points', 'points_smooth', 'boxes', 'flags') + (('keypoints',) if keypoints else ()):
        same_bits(getattr(tr, k)[:, faces], ref[k] if isinstance(ref, dict) else getattr(ref, k).numpy(), '%s %s' % (what, k))


def test_track_equals_the_loop_over_public_calls(world):
    from imm_amd.tracking import OneEuro, Track
    det, frames, reg, ref = world
    tr = det.track(frames, FACES, box_smooth=BETA, one_euro=OneEuro(*OE), fps=FPS)
    assert isinstance(tr, Track) and len(tr) == T and tr.mu.is_cuda and tr.keypoints is None
    assert tuple(tr.mu.shape) == (T, 3, 10, 2) and tuple(tr.boxes.shape) == (T, 3, 4) and tr.boxes.dtype == torch.int32
    assert tuple(tr.lost.shape) == (T, 3) and tr.lost.dtype == torch.bool and tr.outside.dtype == torch.bool
    same_track(tr, ref, 'track')
    assert np.array_equal(ref['boxes'][0], np.array(FACES)[:, 1:]) and np.isfinite(ref['points']).all() and not (ref['flags'] & 1).any()
    print('\nTRACK boxes of face 0 per frame: %s; flags %s' % (ref['boxes'][:, 0].tolist(), ref['flags'].tolist()))
    # with a regressor: the keypoint epilogue of every frame reads the geometry the frame before wrote on the device
    trk = det.track(frames, FACES, regressor=reg, box_smooth=BETA, one_euro=OneEuro(*OE), fps=FPS)
    assert tuple(trk.keypoints.shape) == (T, 3, 5, 2)
    same_track(trk, ref, 'track with a regressor', keypoints=True)


def test_chunks_tracker_repeats_and_a_further_face(world):
    from imm_amd.tracking import OneEuro
    det, frames, reg, ref = world
    kw = dict(box_smooth=BETA, one_euro=OneEuro(*OE), fps=FPS)
    same_track(det.track(frames, FACES, chunk_frames=2, **kw), ref, 'chunk_frames=2')
    same_track(det.track(frames, [f[1:] for f in FACES], chunk_frames=1, **kw), ref, 'chunk_frames=1, four-value boxes')
    same_track(det.track(frames, FACES, **kw), ref, 'a second run')
    live = det.tracker(**kw)
    live.start(frames[0], FACES)
    same_track(live.result(), {k: v[:1] for k, v in ref.items()}, 'tracker after start')
    for f in frames[1:]:
        live.step(f)
    same_track(live.result(), ref, 'tracker')
    small = det.tracker(regressor=reg, **kw)
    small.capacity = 2                                                         # the buffers grow twice on the way
    small.start(frames[0], FACES)
    for f in frames[1:]:
        small.step(f)
    same_track(small.result(), ref, 'tracker with growing buffers', keypoints=True)
    # a further face in the call (same bucket) leaves the others' tracks as they are
    more = det.track(frames, FACES + [FOURTH], **kw)
    assert tuple(more.mu.shape) == (T, 4, 10, 2)
    same_track(more, ref, 'with a fourth face', faces=slice(0, 3))
    # the filter off: points_smooth is points
    off = det.track(frames, FACES, box_smooth=BETA, one_euro=None, fps=FPS).cpu()
    same_bits(off.points_smooth, off.points.numpy(), 'one_euro=None')
    same_bits(off.points, ref['points'], 'one_euro=None points')
    same_bits(off.boxes, ref['boxes'], 'one_euro=None boxes')


def test_detect_is_what_it_was_before_a_track_call(ops):
    cfg, model, eng, P, St = D.make_model(10, 128, 2)
    det = model.landmark_detector(128, max_batch=4)
    frames = clip()
    x = D.images(3, 128, 21)
    before, before_u8 = det.detect(x).cpu(), det.detect(frames[:3]).cpu()
    det.track(frames, FACES)
    assert torch.equal(det.detect(x).cpu(), before) and torch.equal(det.detect(frames[:3]).cpu(), before_u8)
    with pytest.raises(ValueError, match='max_batch'):
        det.track(frames, FACES + [FOURTH] * 2)
    with pytest.raises(RuntimeError, match='start'):
        det.tracker().step(frames[0])


# ----------------------------------------------------------------------------------------------------------------------------
# 3. the script
# ----------------------------------------------------------------------------------------------------------------------------
def test_detect_script_with_track(ops, tmp_path, capsys):
    from PIL import Image
    from imm_amd.inference import LandmarkDetector
    from imm_amd.utils.config import load_configs
    cfg, model, eng, P, St = D.make_model(10, 128, 2)
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, ckpt)
    imdir = tmp_path / 'clip'
    imdir.mkdir()
    frames = clip()
    for i, im in enumerate(frames):
        Image.fromarray(im).save(imdir / ('%03d.png' % i))
    with open(str(tmp_path / 'first.csv'), 'w') as f:
        f.write('file,y0,x0,y1,x1\n' + ''.join('000.png,%d,%d,%d,%d\n' % b[1:] for b in FACES))
    conf = D._write_config(tmp_path, str(tmp_path), str(tmp_path / 'logs'))
    out = str(tmp_path / 'track.npz')
    D._run_script(os.path.join(ROOT, 'scripts', 'detect.py'), ['--configs', conf, '--checkpoint', ckpt, '--images-dir', str(imdir), '--out', out,
                                                               '--batch-size', '4', '--track', '--boxes', str(tmp_path / 'first.csv'),
                                                               '--fps', '30', '--box-smooth', '0.75'])
    assert '5 frames, 3 faces tracked' in capsys.readouterr().out
    r = np.load(out)
    assert list(r['files']) == ['%03d.png' % i for i in range(T)] and r['sizes'].tolist()[1] == [120, 100]
    det = LandmarkDetector.from_checkpoint(load_configs([conf]).model, ckpt, max_batch=4, device=DEV)
    tr = det.track(frames, FACES, box_smooth=0.75, fps=30.0).cpu()
    for k in ('mu', 'points', 'points_smooth', 'boxes', 'flags'):
        same_bits(r[k], getattr(tr, k).numpy(), 'script ' + k)
    np.testing.assert_array_equal(r['landmarks'], (r['mu'] + 1) / 2.0 * 128)
    assert (r['points_smooth'] != r['points']).any()
    D._run_script(os.path.join(ROOT, 'scripts', 'detect.py'), ['--configs', conf, '--checkpoint', ckpt, '--images-dir', str(imdir), '--out', out,
                                                               '--batch-size', '4', '--track', '--boxes', str(tmp_path / 'first.csv'), '--no-filter'])
    r = np.load(out)
    assert np.array_equal(r['points_smooth'], r['points'])
