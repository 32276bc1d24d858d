"""Clip morph on the MI355X: imm_clip_rows and imm_clip_ema in guarded buffers against the numpy restatement of include/imm_clip.h
(tests/clip_reference.py) bit for bit, a lost row through the morph chain at the ops level, LandmarkDetector.morph_clip against the loop
over public calls it replaces (track(), .cpu(), morph() per frame), the filters end to end, chunks and side effects, and the script.

"Bit for bit" compares the stored bits of every element; two NaNs count as equal (test_track_gpu.same_bits)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alignment_reference as AR                  # noqa: E402
import clip_reference as CR                       # noqa: E402
import guarded                                    # noqa: E402
import test_detector_gpu as D                     # noqa: E402  (make_model, _run_script, _write_config)
import test_track_gpu as TG                       # noqa: E402  (same_bits, clip, FACES, OE, FPS, BETA)
import track_reference as TRR                     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
same_bits = TG.same_bits


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


def gin(a):
    return guarded.inp(torch.from_numpy(np.ascontiguousarray(a)), DEV, depth=2)


# ----------------------------------------------------------------------------------------------------------------------------
# 1. imm_clip_rows against the restatement
# ----------------------------------------------------------------------------------------------------------------------------
SPECIAL_ROWS = [(0, -3, -7, -1, 54),                    # a side of 2 (the ramp is <= 0.5 pixels), negative coordinates, a side of 61
                (0, 0, 0, 4194304, 4194304),            # the tracker's largest box
                (0, 5, 5, 5, 9)]                        # an empty box: sy = 0, every landmark of it is not finite


def rows_case(F, K, seed):
    rng = np.random.RandomState(seed)
    h, w = rng.randint(2, 400, F), rng.randint(2, 400, F)
    y0, x0 = rng.randint(-300, 3000, F), rng.randint(-300, 3000, F)
    boxes = np.stack([rng.randint(0, 5, F), y0, x0, y0 + h, x0 + w], axis=1).astype(np.int32)
    boxes[:min(F, 3)] = SPECIAL_ROWS[:min(F, 3)]
    mu = rng.uniform(-1, 1, (F, K, 2)).astype(F32)
    side = (boxes[:, 3:5] - boxes[:, 1:3]).astype(np.float64)
    points = (boxes[:, None, 1:3] + rng.uniform(0, 1, (F, K, 2)) * side[:, None, :]).astype(F32)
    flat = points.reshape(-1, 2)
    flat[0] = (np.nan, np.inf)                                       # a NaN and an inf point: stored as they come out
    if len(flat) > 1:
        f = 1 // K
        flat[1] = (boxes[f, 1] - 10.0 * side[f, 0], boxes[f, 4] + 3.0 * side[f, 1])      # outside the box: the clamp, both ways
    if len(flat) > 2:
        flat[2, 0] = -np.inf
    flags = (2 * rng.randint(0, 2, F)).astype(np.int32)              # bit 1 (the box left the photo) does not drop a row
    if F >= 3:
        flags[1] = 1                                                 # a lost face
    if F >= 65:
        flags[7], flags[64] = 3, 1                                   # and one in the second wave's worth of rows
    mask_feather = rng.uniform(0, 1, F).astype(F32)
    mask_feather[0] = 0.0
    mask_feather[-1] = 1.0
    return boxes, flags, mu, points, mask_feather


@pytest.mark.parametrize('K', [1, 10, 64])
@pytest.mark.parametrize('F', [1, 3, 65])
def test_clip_rows_equals_the_restatement(ops, F, K):
    S = 128
    boxes, flags, mu, points, mask_feather = rows_case(F, K, 100 * F + K)
    for v, (with_points, with_mask, feather) in enumerate(((True, True, 0.125), (False, False, 0.0), (True, False, 0.5), (False, True, 0.25))):
        fl = flags.copy()
        if F == 1 and v % 2:
            fl[0] = 1                                                # the only face, lost
        own, ramp = guarded.out((F, K, 2), torch.float32, DEV), guarded.out((F, 2), torch.float32, DEV)
        soft = guarded.out((F,), torch.float32, DEV) if with_mask else None
        ops.clip_rows(gin(boxes), gin(fl), gin(mu), gin(points) if with_points else None, S, feather, gin(mask_feather) if with_mask else None,
                      own, ramp, soft)
        torch.cuda.synchronize()
        r_own, r_ramp, r_soft = CR.clip_rows(boxes, fl, mu, points if with_points else None, S, feather, mask_feather if with_mask else None)
        what = 'F=%d K=%d points=%s mask=%s feather=%g ' % (F, K, with_points, with_mask, feather)
        same_bits(own, r_own, what + 'own')
        same_bits(ramp, r_ramp, what + 'inv_ramp')
        if with_mask:
            same_bits(soft, r_soft, what + 'inv_soft')
        # the case holds what it says it holds
        lost = (fl & 1) != 0
        assert np.isnan(r_own[lost]).all() and r_ramp[0, 0] == (2.0 if feather <= 0.25 else 1.0), 'a side of 2: a ramp of <= 0.5 pixels'
        if with_points:
            if not lost[0]:
                assert np.isnan(r_own[0, 0, 0]) and r_own[0, 0, 1] == np.inf
            if F * K > 1 and not lost[1 // K]:
                assert r_own.reshape(-1, 2)[1].tolist() == [-1.0, 1.0]
            if F >= 3:
                assert not np.isfinite(r_own[2, :, 0]).any() and np.isfinite(r_own[2, K > 1:, 1]).all(), 'the empty box: H = 0, W = 4'
                assert np.isfinite(r_own[3:][~lost[3:]]).all() if F > 3 else True
        else:
            assert np.array_equal(r_own[~lost].view(np.int32), mu[~lost].view(np.int32))
        if feather == 0.0:
            assert (r_ramp == 2.0).all()


# ----------------------------------------------------------------------------------------------------------------------------
# 2. imm_clip_ema against the restatement
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', [0.25, 1.0])
@pytest.mark.parametrize('width', [6, 48, 768])
@pytest.mark.parametrize('n', [1, 3, 65])
def test_clip_ema_equals_the_restatement(ops, n, width, alpha):
    rng = np.random.RandomState(1000 * n + width)
    T = 4
    xs = rng.uniform(-100, 100, (T, n, width)).astype(F32)
    xs[3, 0, 1] = np.nan                                             # a NaN in x enters the state
    skip, lost = np.zeros((T, n), np.int32), np.zeros((T, n), np.int32)
    skip[0, 0] = 5                                                   # skipped on the first frame: its seen stays 0
    skip[2, n // 2] = 1                                              # skipped mid-clip
    lost[1, n - 1] = 3                                               # lost
    lost[:, 0] |= 2                                                  # bit 1 alone does not skip
    if n >= 65:
        xs[1, 64, width - 1] = np.nan
        skip[1, 33], lost[2, 64] = 2, 1
    state, seen = guarded.out((n, width), torch.float32, DEV), guarded.out((n,), torch.int32, DEV, fill=0)
    r_state, r_seen = np.full((n, width), np.nan, F32), np.zeros(n, np.int32)
    r_state.view(np.int32)[:] = -1                                   # the guarded buffer's bytes: a skipped row leaves them alone
    for t in range(T):
        x = gin(xs[t])
        lost_t = None if t == 3 else lost[t]                         # the last frame runs without the tracker's flags
        ops.clip_ema(x, state, seen, gin(skip[t]), None if lost_t is None else gin(lost_t), alpha)
        torch.cuda.synchronize()
        r_x = xs[t].copy()
        CR.clip_ema(r_x, r_state, r_seen, skip[t], lost_t, alpha)
        what = 'n=%d width=%d alpha=%g frame %d ' % (n, width, alpha, t)
        same_bits(x, r_x, what + 'x')
        same_bits(state, r_state, what + 'state')
        same_bits(seen, r_seen, what + 'seen')
        if t == 0:
            assert r_seen[0] == 0 and (r_seen[1:] == 1).all(), 'the skipped row has seen nothing'
    assert r_seen.all() and np.isnan(r_state[0, 1]) and np.isfinite(r_state[0, 2:]).all()


# ----------------------------------------------------------------------------------------------------------------------------
# 3. a lost row through the chain, at the ops level
# ----------------------------------------------------------------------------------------------------------------------------
def chain(ops, photo, donor, boxes, track_flags, mu, points, lm_b, K, m, B):
    """clip_rows -> morph_poses -> hull_fit -> warp_fit -> seam_fit -> morph_paste over these rows of ONE photo: (canvas u8, fit flags,
    hull flags, seam flags, own) on the host."""
    from imm_amd import generation as GN
    from imm_amd import morphing as MP
    from imm_amd import warping as WP
    from imm_amd.inference import pack_u8
    n, M = len(boxes), K + 4 * m
    src, offs_d, hw_d, _b = pack_u8([photo], DEV)
    don, doffs_d, dhw_d, dboxes_d = pack_u8([donor], DEV, np.array([(0, 0, 0) + donor.shape[:2]] * n, np.int32))
    canvas = src.clone()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    z = lambda *shape, **kw: torch.empty(*shape, device=DEV, **kw)
    boxes_d, own, ramp, soft = dev(boxes), guarded.out((n, K, 2), torch.float32, DEV), z(n, 2), z(n)
    ops.clip_rows(boxes_d, dev(track_flags), dev(mu), dev(points), 128, 0.125, dev(np.full(n, 0.1, F32)), own, ramp, soft)
    p2, m2 = z(2, n, K, 2), z(2, n, K, 2)
    ops.morph_poses(own, dev(lm_b), dev(np.zeros(n, F32)), p2, m2)
    grow, edges, hflags = dev(np.full(n, 1.25, F32)), z(n, K, 3), z(n, dtype=torch.int32)
    ops.hull_fit(p2[0], boxes_d, grow, edges, hflags)
    c2, t2, f2 = z(2, n, M + 3, 2), z(2, n, M, 2), z(2, n, dtype=torch.int32)
    ops.warp_fit(p2.view(2 * n, K, 2), m2.view(2 * n, K, 2), dev(WP.warp_anchors(m).astype(F32)), 1.0, 0.0, c2.view(2 * n, M + 3, 2),
                 t2.view(2 * n, M, 2), f2.view(2 * n))
    texture, ring, diff, sflags = dev(np.ones(n, F32)), z(n, B, 2), z(n, B, 3), z(n, dtype=torch.int32)
    ops.seam_fit(p2[0], boxes_d, grow, edges, hflags, dev(MP.seam_dirs(B)), src, offs_d, hw_d, don, doffs_d, dhw_d, dboxes_d, texture, t2[0],
                 c2[0], c2[1], None, ring, diff, sflags)
    area = int(((boxes[:, 3] - boxes[:, 1]) * (boxes[:, 4] - boxes[:, 2])).max())
    ops.morph_paste(src, canvas, offs_d, hw_d, don, doffs_d, dhw_d, boxes_d, dboxes_d, dev(GN.compose_links(boxes)), ramp, texture, t2[0],
                    c2[0], c2[1], area, edges=edges, inv_soft=soft, ring=ring, diff=diff, seamless=dev(np.ones(n, F32)))
    torch.cuda.synchronize()
    return (canvas.cpu().numpy()[:photo.size].reshape(photo.shape), (f2[0] | f2[1]).cpu().numpy(), hflags.cpu().numpy(), sflags.cpu().numpy(),
            own.cpu().numpy())


def test_a_lost_row_is_dropped_by_the_chain(ops):
    """Three overlapping rows of one photo, the middle one lost: its NaN landmarks flag the fit, the hull and the seam, and the canvas
    is the canvas of the two other rows alone, bit for bit."""
    K, m, B = 10, 2, 32
    rng = np.random.RandomState(3)
    photo = AR.smooth_photo(96, 110, 3)
    donor = (AR.smooth_photo(60, 50, 5) * 0.6 + 40).astype(np.uint8)
    boxes = np.array([(0, 4, 6, 64, 56), (0, 20, 30, 84, 88), (0, 30, 50, 92, 108)], np.int32)
    mu = rng.uniform(-0.7, 0.7, (3, K, 2)).astype(F32)
    lm_b = rng.uniform(-0.7, 0.7, (3, K, 2)).astype(F32)
    st = TRR.new_state(3, K)
    points = TRR.track_step(mu, boxes, [photo.shape[:2]], st, 128, 0, 1, 0.5, None, 25.0)[0]
    flags = np.array([0, 1, 2], np.int32)
    canvas, fit, hull, seam, own = chain(ops, photo, donor, boxes, flags, mu, points, lm_b, K, m, B)
    keep = [0, 2]
    canvas2, fit2, hull2, seam2, own2 = chain(ops, photo, donor, boxes[keep], flags[keep], mu[keep], points[keep], lm_b[keep], K, m, B)
    assert np.isnan(own[1]).all() and np.isfinite(own[keep]).all()
    same_bits(own[keep], own2, 'own of the rows that stay')
    assert fit[1] & 1 and hull[1] != 0 and seam[1] != 0, (fit, hull, seam)
    assert not fit[keep].any() and not hull[keep].any() and not seam[keep].any() and not (fit2.any() or hull2.any() or seam2.any())
    assert np.array_equal(canvas, canvas2), 'the lost row wrote nothing'
    changed = (canvas != photo).any(axis=2)
    assert changed[4:64, 6:56].sum() > 300 and changed[30:92, 50:108].sum() > 300, 'the two other rows were pasted'
    alone = np.zeros_like(changed)
    alone[20:84, 30:88] = True
    alone[4:64, 6:56] = False
    alone[30:92, 50:108] = False
    assert alone.sum() > 100 and not changed[alone].any(), 'the lost row\'s own pixels are the photo\'s'


# ----------------------------------------------------------------------------------------------------------------------------
# 4. morph_clip against the loop over public calls
# ----------------------------------------------------------------------------------------------------------------------------
FACES = TG.FACES
DONOR_BOXES = [(0, 0, 0, 70, 60), (1, 0, 0, 64, 72), (0, 6, 4, 66, 52)]
RING = 32
GROW = 16.0               # the landmarks of this untrained model lie within a pixel of each other: the hull is grown as far as grow goes
PASTES = {'plain': dict(), 'colour': dict(colour=1.0), 'hull': dict(mask='hull', grow=GROW),
          'seam': dict(mask='hull', grow=GROW, seamless=1.0, colour=0.5)}


def donor_photos():
    return [(AR.smooth_photo(70, 60, 5) * 0.6 + 50).astype(np.uint8), (255 - AR.smooth_photo(64, 72, 7) * 0.7).astype(np.uint8)]


@pytest.fixture(scope='module')
def world(ops):
    """One model and detector (K = 10, S = 128, max_batch 4), the clip of test_track_gpu with its three faces, two small donor photos and
    their landmarks taken once, and the reference track."""
    from imm_amd.tracking import OneEuro
    cfg, model, eng, P, St = D.make_model(10, 128, 2)
    det = model.landmark_detector(128, max_batch=4)
    frames, donors = TG.clip(), donor_photos()
    dl = det.landmarks(donors, DONOR_BOXES).clone()
    kw = dict(box_smooth=TG.BETA, one_euro=OneEuro(*TG.OE), fps=TG.FPS)
    tr = det.track(frames, FACES, **kw).cpu()
    return dict(det=det, frames=frames, donors=donors, dl=dl, kw=kw, track=tr, loops={})


def public_loop(world, smooth, paste):
    """The loop morph_clip replaces: track(), .cpu(), then morph() per frame with that frame's boxes and landmarks."""
    key = (smooth, paste)
    if key not in world['loops']:
        det, tr, S = world['det'], world['track'], world['det'].S
        outs, pms = [], []
        for t, frame in enumerate(world['frames']):
            rows = np.concatenate([np.zeros((len(FACES), 1), np.int32), tr.boxes[t].numpy()], axis=1)
            own = CR.clip_rows(rows, tr.flags[t].numpy(), tr.mu[t].numpy(), tr.points_smooth[t].numpy(), S, 0.125, None)[0] if smooth \
                else tr.mu[t].numpy()
            out, pm = det.morph([frame], world['donors'], boxes=rows.tolist(), donor_boxes=DONOR_BOXES, shape=0.0, texture=1.0, feather=0.125,
                                landmarks=torch.from_numpy(own), donor_landmarks=world['dl'], return_transform=True, ring=RING, **PASTES[paste])
            outs.append(out[0].cpu().numpy())
            pms.append(pm)
        world['loops'][key] = (outs, pms)
    return world['loops'][key]


def host(t):
    return None if t is None else t.cpu().numpy()


@pytest.mark.parametrize('paste', list(PASTES))
@pytest.mark.parametrize('smooth', [False, True])
def test_morph_clip_equals_the_loop_over_public_calls(world, smooth, paste):
    from imm_amd.clip import ClipMorph
    det, frames, tr = world['det'], world['frames'], world['track']
    T, Fn = len(frames), len(FACES)
    # what the comparison rests on
    assert not tr.lost.any(), 'no face of the reference track is lost'
    outs, pms = public_loop(world, smooth, paste)
    print('\nCLIP MORPH smooth=%s %s: bytes changed per frame %s' % (smooth, paste, [int((o != f).sum()) for o, f in zip(outs, frames)]))
    assert all((o != f).any() for o, f in zip(outs, frames)), 'every frame is changed by the paste'
    cm = det.morph_clip(frames, FACES, world['donors'], donor_boxes=DONOR_BOXES, donor_landmarks=world['dl'], smooth=smooth, colour_smooth=1,
                        seam_smooth=1, ring=RING, **dict(world['kw'], **PASTES[paste]))
    assert isinstance(cm, ClipMorph) and len(cm) == T and len(cm.frames) == T and cm.own.is_cuda
    assert tuple(cm.own.shape) == (T, Fn, 10, 2) and tuple(cm.fit_flags.shape) == (T, Fn) and cm.fit_flags.dtype == torch.int32
    TG.same_track(cm.track, tr, 'the clip\'s track')
    matched, hull, seam = 'colour' in PASTES[paste], 'mask' in PASTES[paste], 'seamless' in PASTES[paste]
    assert (cm.colour_gain is not None) == matched == (cm.colour_flags is not None)
    assert (cm.hull_flags is not None) == hull and (cm.seam_diff is not None) == seam == (cm.seam_flags is not None)
    for t in range(T):
        what = 'smooth=%s %s frame %d ' % (smooth, paste, t)
        assert cm.frames[t].dtype == torch.uint8 and tuple(cm.frames[t].shape) == frames[t].shape
        same_bits(cm.frames[t], outs[t], what + 'bytes')
        pm = pms[t]
        same_bits(cm.own[t], host(pm.mu), what + 'own')
        same_bits(cm.fit_flags[t], host(pm.flags), what + 'fit_flags')
        if matched:
            same_bits(cm.colour_gain[t], host(pm.colour_gain), what + 'colour_gain')
            same_bits(cm.colour_flags[t], host(pm.colour_flags), what + 'colour_flags')
        if hull:
            same_bits(cm.hull_flags[t], host(pm.hull_flags), what + 'hull_flags')
        if seam:
            same_bits(cm.seam_diff[t], host(pm.seam_diff), what + 'seam_diff')
            same_bits(cm.seam_flags[t], host(pm.seam_flags), what + 'seam_flags')
    if smooth:
        assert (host(cm.own) != tr.mu.numpy()).any(), 'the filtered points are not the pose head\'s'
    else:
        same_bits(cm.own, tr.mu.numpy(), 'own is mu')


# ----------------------------------------------------------------------------------------------------------------------------
# 5. the filters, end to end
# ----------------------------------------------------------------------------------------------------------------------------
def test_filters_end_to_end(world):
    det, frames, tr = world['det'], world['frames'], world['track']
    call = lambda **kw: det.morph_clip(frames, FACES, world['donors'], donor_boxes=DONOR_BOXES, donor_landmarks=world['dl'], ring=RING,
                                       **dict(world['kw'], **kw))
    flags = tr.flags.numpy()
    # the colour gain
    raw = call(colour=1.0, colour_smooth=1)
    gains = host(raw.colour_gain)
    assert (gains[0] != gains[1]).any() and (gains[1] != gains[3]).any(), 'the raw gains differ from frame to frame: the filter has work'
    fil = call(colour=1.0, colour_smooth=0.25)
    same_bits(fil.colour_gain, CR.ema_frames(gains, host(raw.colour_flags), flags, 0.25), 'the filtered gain')
    same_bits(fil.colour_flags, host(raw.colour_flags), 'colour_flags')
    same_bits(fil.frames[0], host(raw.frames[0]), 'frame 0 passes')
    assert any((host(a) != host(b)).any() for a, b in zip(fil.frames[1:], raw.frames[1:])), 'a later frame is pasted with the filtered gain'
    assert fil.seam_diff is None and fil.hull_flags is None
    # the membrane's differences
    seam = dict(colour=1.0, colour_smooth=1, mask='hull', grow=GROW, seamless=1.0)
    raw = call(seam_smooth=1, **seam)
    diffs = host(raw.seam_diff)
    assert tuple(diffs.shape) == (len(frames), len(FACES), RING, 3) and (diffs[0] != diffs[1]).any() and not host(raw.seam_flags).any()
    fil = call(seam_smooth=0.25, **seam)
    same_bits(fil.seam_diff, CR.ema_frames(diffs, host(raw.seam_flags), flags, 0.25), 'the filtered differences')
    same_bits(fil.colour_gain, host(raw.colour_gain), 'the gain is not filtered at colour_smooth = 1')
    same_bits(fil.frames[0], host(raw.frames[0]), 'frame 0 passes')
    assert any((host(a) != host(b)).any() for a, b in zip(fil.frames[1:], raw.frames[1:])), 'a later frame is pasted with the filtered differences'


# ----------------------------------------------------------------------------------------------------------------------------
# 6. chunks and side effects
# ----------------------------------------------------------------------------------------------------------------------------
FIELDS = ('own', 'fit_flags', 'colour_gain', 'colour_flags', 'hull_flags', 'seam_diff', 'seam_flags')


def same_clip(got, ref, what):
    assert len(got) == len(ref)
    for t in range(len(ref)):
        same_bits(got.frames[t], host(ref.frames[t]), '%s frame %d' % (what, t))
    for k in FIELDS:
        same_bits(getattr(got, k), host(getattr(ref, k)), '%s %s' % (what, k))
    TG.same_track(got.track, ref.track.cpu(), what + ' track')


def test_chunks_repeats_and_side_effects(world):
    det, frames = world['det'], world['frames']
    x = D.images(3, 128, 21)
    before, before_u8, track_before = det.detect(x).cpu(), det.detect(frames[:3]).cpu(), det.track(frames, FACES, **world['kw']).cpu()
    kw = dict(donor_boxes=DONOR_BOXES, donor_landmarks=world['dl'], ring=RING, colour=0.75, mask='hull', grow=GROW, seamless=[1.0, 0.5, 0.0],
              **world['kw'])
    ref = det.morph_clip(frames, FACES, world['donors'], **kw)
    kept = [host(f).copy() for f in ref.frames]
    for chunk in (1, 2):
        same_clip(det.morph_clip(frames, [f[1:] for f in FACES], world['donors'], chunk_frames=chunk, **kw), ref, 'chunk_frames=%d' % chunk)
    same_clip(det.morph_clip(frames, FACES, world['donors'], chunk_frames=32, **kw), ref, 'a second call')
    assert all(np.array_equal(host(f), k) for f, k in zip(ref.frames, kept)), 'the first call\'s result is left alone'
    # ONE donor for all, its landmarks detected by the call
    one = det.morph_clip(frames, FACES, world['donors'][:1], **world['kw'])
    assert one.colour_gain is None and all((host(f) != g).any() for f, g in zip(one.frames, frames))
    assert torch.equal(det.detect(x).cpu(), before) and torch.equal(det.detect(frames[:3]).cpu(), before_u8)
    TG.same_track(det.track(frames, FACES, **world['kw']), track_before, 'track after morph_clip')
    with pytest.raises(ValueError, match='max_batch'):
        det.morph_clip(frames, FACES + [TG.FOURTH] * 2, world['donors'][:1])
    with pytest.raises(ValueError, match="needs mask='hull'"):
        det.morph_clip(frames, FACES, world['donors'][:1], seamless=1.0)


# ----------------------------------------------------------------------------------------------------------------------------
# 7. the script
# ----------------------------------------------------------------------------------------------------------------------------
def test_generate_script_morphs_a_clip(ops, tmp_path, capsys):
    from PIL import Image
    from imm_amd.inference import LandmarkDetector
    from imm_amd.utils.config import load_configs
    cfg, model, eng, P, St = D.make_model(10, 128, 2)
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, ckpt)
    imdir, donor_dir = tmp_path / 'clip', tmp_path / 'donors'
    imdir.mkdir()
    donor_dir.mkdir()
    frames, donors = TG.clip(), donor_photos()
    for i, im in enumerate(frames):
        Image.fromarray(im).save(imdir / ('%03d.png' % i))
    for name, im in zip('ab', donors):
        Image.fromarray(im).save(donor_dir / (name + '.png'))
    with open(str(tmp_path / 'first.csv'), 'w') as f:
        f.write('file,y0,x0,y1,x1\n' + ''.join('000.png,%d,%d,%d,%d\n' % b[1:] for b in FACES))
    with open(str(tmp_path / 'donors.csv'), 'w') as f:
        f.write('file,y0,x0,y1,x1\n' + ''.join('%s.png,%d,%d,%d,%d\n' % (('ab'[b[0]],) + b[1:]) for b in DONOR_BOXES))
    conf = D._write_config(tmp_path, str(tmp_path), str(tmp_path / 'logs'))
    script = os.path.join(ROOT, 'scripts', 'generate.py')
    out_dir = str(tmp_path / 'out')
    argv = ['--configs', conf, '--checkpoint', ckpt, '--appearance-dir', str(imdir), '--boxes', str(tmp_path / 'first.csv'), '--batch-size', '4',
            '--morph', '--clip', '--donor-dir', str(donor_dir), '--donor-boxes', str(tmp_path / 'donors.csv'), '--shape', '0', '--texture', '1',
            '--colour', '1', '--mask', 'hull', '--grow', '16', '--seamless', '0.75', '--ring', '32', '--colour-smooth', '0.5', '--fps', '30']
    D._run_script(script, argv + ['--out-dir', out_dir])
    assert '5 frames, 3 faces morphed (0 lost) ->' in capsys.readouterr().out
    det = LandmarkDetector.from_checkpoint(load_configs([conf]).model, ckpt, max_batch=4, device=DEV)
    cm = det.morph_clip(frames, FACES, donors, donor_boxes=DONOR_BOXES, shape=0.0, texture=1.0, colour=1.0, mask='hull', grow=16.0, seamless=0.75, ring=32,
                        colour_smooth=0.5, fps=30.0)
    assert sorted(os.listdir(out_dir)) == ['%03d.png' % i for i in range(len(frames))]
    for i, want in enumerate(cm.frames):
        png = np.asarray(Image.open(os.path.join(out_dir, '%03d.png' % i)))
        assert np.array_equal(png, host(want)), i
        assert (png != frames[i]).any()
    with pytest.raises(ValueError, match='--clip'):
        D._run_script(script, argv + ['--steps', '3', '--out-dir', str(tmp_path / 'no')])
    with pytest.raises(ValueError, match='go with --morph --clip'):
        D._run_script(script, [a for a in argv if a != '--clip'] + ['--out-dir', str(tmp_path / 'no')])
    assert not os.path.exists(str(tmp_path / 'no'))
