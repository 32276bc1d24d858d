"""Landmark quality on the MI355X: imm_landmark_scores in guarded buffers against the numpy restatement of include/imm_score.h
(tests/score_reference.py) bit for bit, LandmarkDetector.quality against the restatement fed with its own marginals, the tracker with
a gate against the loop over public calls (quality() per frame, the restatement, tests/track_reference.py on the gated landmarks), the
ungated paths with the new kernel made unreachable, clip morph with a gate, and the scripts.

"Bit for bit": see score_reference.same: a NaN in the same place counts as equal in computed values; copies are compared as bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alignment_reference as AR                  # noqa: E402
import guarded                                    # noqa: E402
import score_reference as SR                      # noqa: E402
import test_detector_gpu as D                     # noqa: E402  (make_model, images, _run_script, _write_config)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 128
OE = (1.0, 0.05, 1.0)
FPS = 25.0
BETA = 0.5


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


def host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def gin(a):
    return guarded.inp(torch.from_numpy(np.ascontiguousarray(a)), DEV, depth=2)


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the restatement, 2. nothing written outside the outputs
# ----------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 2, 2), (3, 10, 16, 16), (5, 30, 32, 16), (70, 64, 32, 32)]


def run_kernel(ops, case, shared, max_spread, max_residual, blank, with_mu_out=True):
    py, px, mu, boxes, ref = case
    F, K = mu.shape[:2]
    py_d, px_d, mu_d = gin(py), gin(px), gin(mu)
    boxes_d = None if boxes is None else gin(boxes)
    ref_d = gin(ref)
    out = dict(spread=guarded.out((F, K), torch.float32, DEV), score=guarded.out((F, 2), torch.float32, DEV),
               qflags=guarded.out((F,), torch.int32, DEV), mu_out=guarded.out((F, K, 2), torch.float32, DEV) if with_mu_out else None)
    # a shared reference [K, 2] at stride 0; per-face references inside a state-sized buffer, as the tracker passes them
    ref_arg, stride = (ref_d, 0) if shared else (ref_d.view(-1)[5:], 5 + 6 * K)
    ops.landmark_scores(py_d, px_d, mu_d, boxes_d, ref_arg, stride, S, max_spread, max_residual, blank, out['spread'], out['score'],
                        out['qflags'], out['mu_out'])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('shared', [False, True], ids=['boxes_per_face_ref', 'no_boxes_shared_ref'])
@pytest.mark.parametrize('F,K,h,w', SHAPES, ids=['%dx%dx%dx%d' % s for s in SHAPES])
def test_landmark_scores_equals_the_restatement(ops, F, K, h, w, shared):
    case, ref_np, ts, tr = SR.kernel_case_checked(F, K, h, w, shared)
    py, px, mu, boxes, ref = case
    for blank in (1, 0):
        want = SR.landmark_scores(py, px, mu, boxes, ref_np, S, ts, tr, blank)
        got = run_kernel(ops, case, shared, ts, tr, blank)
        what = 'F=%d K=%d h=%d w=%d shared=%s blank=%d ' % (F, K, h, w, shared, blank)
        SR.same(host(got['spread']), want[0], what + 'spread')
        SR.same(host(got['score']), want[1], what + 'score')
        SR.same(host(got['qflags']), want[2], what + 'qflags')
        SR.same_bits(host(got['mu_out']), want[3], what + 'mu_out')


def test_mu_out_may_be_null_without_blank_and_refusals_launch_nothing(ops):
    from imm_amd._lib import ImmHipError
    F, K, h, w = 3, 10, 16, 16
    case = SR.kernel_case(F, K, h, w, 5, True)
    py, px, mu, _b, ref = case
    want = SR.landmark_scores(py, px, mu, None, ref, S)
    got = run_kernel(ops, case, True, None, None, 0, with_mu_out=False)
    SR.same(host(got['spread']), want[0], 'mu_out NULL spread')
    SR.same(host(got['score']), want[1], 'mu_out NULL score')
    SR.same(host(got['qflags']), want[2], 'mu_out NULL qflags')
    # without a reference: residual 0
    none = SR.landmark_scores(py, px, mu, None, None, S)
    o = dict(spread=guarded.out((F, K), torch.float32, DEV), score=guarded.out((F, 2), torch.float32, DEV), qflags=guarded.out((F,), torch.int32, DEV))
    ops.landmark_scores(gin(py), gin(px), gin(mu), None, None, 0, S, None, None, 0, o['spread'], o['score'], o['qflags'], None)
    torch.cuda.synchronize()
    SR.same(host(o['score']), none[1], 'no reference')
    assert (none[1][[0], 1] == 0).all()

    def refused(match, K=K, h=h, max_spread=None, blank=0, mu_out=True):
        spread, score, qflags = guarded.out((F, K), torch.float32, DEV), guarded.out((F, 2), torch.float32, DEV), guarded.out((F,), torch.int32, DEV)
        mo = guarded.out((F, K, 2), torch.float32, DEV) if mu_out else None
        z = lambda *shape: guarded.out(shape, torch.float32, DEV, fill=0.0)
        with pytest.raises(ImmHipError, match=match):
            ops.landmark_scores(z(F, h, K), z(F, w, K), z(F, K, 2), None, None, 0, S, max_spread, None, blank, spread, score, qflags, mo)
        torch.cuda.synchronize()
        assert all(guarded.untouched(t) for t in (spread, score, qflags) + ((mo,) if mu_out else ())), 'a refused call launched'

    refused('1 <= K <= 64', K=65)
    refused('2 <= h, w <= 64', h=1)
    refused('NaN', max_spread=float('nan'))
    refused('mu_out', blank=1, mu_out=False)
    refused('blank', blank=2)


# ----------------------------------------------------------------------------------------------------------------------------
# 3. LandmarkDetector.quality
# ----------------------------------------------------------------------------------------------------------------------------
def photos():
    return [AR.smooth_photo(96, 80, 3), AR.smooth_photo(120, 100, 4), AR.smooth_photo(96, 80, 5)]


PHOTO_BOXES = [(0, 10, 8, 70, 60), (0, 30, 20, 90, 75), (1, -10, -6, 50, 40), (1, 40, 30, 118, 96), (2, 0, 0, 96, 80), (2, 20, 10, 80, 70)]


@pytest.fixture(scope='module')
def world(ops):
    """One model and detector (K = 10, S = 128, heat maps 16 x 16, max_batch 4) and a template."""
    from imm_amd.alignment import LandmarkTemplate
    cfg, model, eng, P, St = D.make_model(10, 128, 2)
    det = model.landmark_detector(128, max_batch=4)
    tpl = LandmarkTemplate(np.random.RandomState(2).uniform(-0.7, 0.7, (10, 2)), 128)
    return dict(det=det, tpl=tpl, cache={})


def test_quality_equals_the_restatement_on_its_own_marginals(world):
    from imm_amd.quality import LandmarkQuality, QualityGate
    det, tpl = world['det'], world['tpl']
    ims, x = photos(), D.images(5, 128, 21)
    before = det.detect(x).cpu()
    for name, images, boxes, mu_ref in (('photos with boxes', ims, PHOTO_BOXES, lambda: det.landmarks(ims, PHOTO_BOXES)),
                                        ('photos', ims, None, lambda: det.detect(ims)), ('tensor batch', x, None, lambda: det.detect(x))):
        n = len(boxes) if boxes is not None else len(images)
        for template in (None, tpl):
            q = det.quality(images, boxes, template=template)
            assert isinstance(q, LandmarkQuality) and len(q) == n and q.mu.is_cuda and q.S == 128
            assert tuple(q.spread.shape) == (n, 10) and tuple(q.score.shape) == (n, 2) and tuple(q.py.shape) == (n, 16, 10) == tuple(q.px.shape)
            c = q.cpu()
            py, px, mu = c.py.numpy(), c.px.numpy(), c.mu.numpy()
            want = SR.landmark_scores(py, px, mu, None, None if template is None else tpl.points, S)
            what = '%s, template %s: ' % (name, template is not None)
            SR.same(c.spread.numpy(), want[0], what + 'spread')
            SR.same(c.score.numpy(), want[1], what + 'score')
            SR.same(c.flags.numpy(), want[2], what + 'flags')
            SR.same_bits(mu, host(mu_ref()), what + 'mu is detect()\'s')
            assert np.isfinite(want[1]).all() and (want[2] == 0).all() and not c.unsure.any()
            assert (want[1][:, 1] == 0).all() if template is None else (want[1][:, 1] > 0).all()
            assert np.allclose(py.sum(1), 1, atol=1e-3) and np.allclose(px.sum(1), 1, atol=1e-3), 'the marginals are probabilities'
            # a gate sets the flags by the same rule; a score equal to its threshold passes
            ts = float(np.sort(want[4])[n // 2])
            tr = None if template is None else float(np.sort(want[5])[n // 2])
            g = det.quality(images, boxes, template=template, gate=QualityGate(ts, tr)).cpu()
            wg = SR.landmark_scores(py, px, mu, None, None if template is None else tpl.points, S, ts, tr)
            SR.same(g.flags.numpy(), wg[2], what + 'flags with a gate')
            SR.same_bits(g.mu.numpy(), mu, what + 'stills are never blanked')
            assert (wg[2] != 0).any() and (wg[2] == 0).any() and g.unsure.tolist() == (wg[2] != 0).tolist()
    assert torch.equal(det.detect(x).cpu(), before), 'detect() returns what it returned before'
    with pytest.raises(ValueError, match='QualityGate'):
        det.quality(x, gate=0.5)
    with pytest.raises(ValueError, match='K = 30'):
        det.quality(x, gate=QualityGate(0.5, K=30, S=128))


# ----------------------------------------------------------------------------------------------------------------------------
# 4. the tracker with a gate
# ----------------------------------------------------------------------------------------------------------------------------
T = 6
FACES = [(0, 4, 4, 44, 38), (0, 50, 6, 92, 42), (0, 20, 44, 72, 78)]
FIELDS = ('mu', 'points', 'points_smooth', 'boxes', 'flags')


def clip():
    """Six frames of two sizes cut from one smooth photo, each shifted a few pixels from the last."""
    big = AR.smooth_photo(150, 130, 3)
    frames = []
    for t in range(T):
        h, w = ((96, 80), (120, 100))[t % 2]
        oy, ox = 4 + 3 * t, 20 - 2 * t
        frames.append(np.ascontiguousarray(big[oy:oy + h, ox:ox + w]))
    return frames


def same_track(tr, ref, what, scores=True):
    tr = tr.cpu()
    get = lambda k: ref[k] if isinstance(ref, dict) else host(getattr(ref, k))
    for k in FIELDS:
        SR.same(host(getattr(tr, k)), get(k), '%s %s' % (what, k))
    if scores:
        for k in ('spread', 'score', 'qflags'):
            SR.same(host(getattr(tr, k)), get(k), '%s %s' % (what, k))


def tracked(world):
    """The clip tracked without a gate, with an open gate and with the chosen one, and the loops over public calls, made once."""
    c = world['cache']
    if 'plain' in c:
        return c
    from imm_amd.quality import QualityGate
    from imm_amd.tracking import OneEuro
    det = world['det']
    frames = clip()
    kw = dict(box_smooth=BETA, one_euro=OneEuro(*OE), fps=FPS)

    def observe(t, rows):
        q = det.quality([frames[t]], rows.tolist()).cpu()
        return q.py.numpy(), q.px.numpy(), q.mu.numpy()
    sizes = [f.shape[:2] for f in frames]
    c.update(frames=frames, kw=kw, observe=observe, sizes=sizes)
    c['plain'] = det.track(frames, FACES, **kw).cpu()
    c['open'] = det.tracker(gate=QualityGate(), **kw).track(frames, FACES).cpu()
    c['open_ref'] = SR.gated_track(observe, sizes, FACES, S, (None, None), BETA, OE, FPS)
    # max_spread: the midpoint of two adjacent distinct sorted f64 mean spreads of frames 1 and later, the upper one the widest face of
    # frame 1: that face is blanked on frame 1 (whose landmarks do not depend on the gate) and the other two are kept
    sbar = c['open_ref']['sbar']
    v = np.unique(sbar[1:])
    i = int(np.searchsorted(v, sbar[1].max()))
    assert i >= 1, 'frame 1 holds two distinct mean spreads'
    thr = (v[i - 1] + v[i]) / 2
    assert v[i - 1] < thr < v[i]
    c['thr'], c['gate'] = thr, QualityGate(max_spread=float(thr))
    c['gated'] = det.tracker(gate=c['gate'], **kw).track(frames, FACES).cpu()
    c['gated_ref'] = SR.gated_track(observe, sizes, FACES, S, (thr, None), BETA, OE, FPS)
    return c


def test_an_open_gate_scores_and_changes_nothing(world):
    c = tracked(world)
    plain, opened = c['plain'], c['open']
    assert plain.spread is None and plain.qflags is None and not plain.unsure.any() and tuple(plain.unsure.shape) == (T, 3)
    same_track(opened, plain, 'gate=QualityGate() against no gate', scores=False)
    same_track(opened, c['open_ref'], 'gate=QualityGate() against the loop')
    assert tuple(opened.spread.shape) == (T, 3, 10) and tuple(opened.score.shape) == (T, 3, 2) and opened.qflags.dtype == torch.int32
    assert not opened.unsure.any() and (opened.score[0, :, 1] == 0).all() and torch.isfinite(opened.score).all()
    print('\nGATE mean spread per frame and face: %s' % np.array2string(c['open_ref']['sbar'], precision=6))


def test_a_gate_equals_the_loop_over_public_calls(world):
    from imm_amd.quality import QualityGate
    c = tracked(world)
    det, frames, kw, gated, ref = world['det'], c['frames'], c['kw'], c['gated'], c['gated_ref']
    same_track(gated, ref, 'gated track against the loop')
    blanked = ref['qflags'][1:] != 0
    print('\nGATE max_spread %.9g blanks (frame, face) %s' % (c['thr'], [(int(t) + 1, int(f)) for t, f in np.argwhere(blanked)]))
    assert blanked.any() and (~blanked).any(), 'at least one later (frame, face) is blanked and at least one is kept'
    assert blanked[0].sum() == 1, 'the widest face of frame 1'
    unsure, lost = host(gated.unsure), host(gated.lost)
    assert np.array_equal(unsure[1:], blanked) and np.array_equal(lost[1:], blanked) and not lost[0].any()
    boxes, points, mu = host(gated.boxes), host(gated.points), host(gated.mu)
    for t, f in np.argwhere(unsure):
        if t == 0:
            continue
        assert np.isnan(points[t, f]).all() and np.isfinite(mu[t, f]).all(), 'the points are NaN, the raw landmarks are reported'
        if t + 1 < T:
            assert np.array_equal(boxes[t + 1, f], boxes[t, f]), 'the frame after a blanked one is cut with the same box'
    assert np.isfinite(points[~unsure]).all()
    # frame 0 is never blanked, even when its bit is set: a gate nothing passes
    shut = det.tracker(gate=QualityGate(max_spread=1e-6), **kw).track(frames, FACES).cpu()
    assert shut.unsure.all() and not shut.lost[0].any() and shut.lost[1:].all() and torch.isfinite(shut.points[0]).all()
    assert all(torch.equal(shut.boxes[t], shut.boxes[1]) for t in range(2, T))
    # chunks, the live tracker, growing buffers
    same_track(det.tracker(gate=c['gate'], **kw).track(frames, FACES, chunk_frames=2), ref, 'chunk_frames=2')
    live = det.tracker(gate=c['gate'], **kw)
    live.capacity = 2                                                          # the buffers grow twice on the way
    live.start(frames[0], FACES)
    same_track(live.result(), {k: v[:1] for k, v in ref.items()}, 'tracker after start')
    for f in frames[1:]:
        live.step(f)
    same_track(live.result(), ref, 'tracker with growing buffers')
    with pytest.raises(ValueError, match='QualityGate'):
        det.tracker(gate=0.5)
    with pytest.raises(ValueError, match='S = 64'):
        det.tracker(gate=QualityGate(0.5, K=10, S=64))


# ----------------------------------------------------------------------------------------------------------------------------
# 5. gate=None is the code of before, 6. clip morph
# ----------------------------------------------------------------------------------------------------------------------------
DONOR_BOXES = [(0, 0, 0, 70, 60), (1, 0, 0, 64, 72), (0, 6, 4, 66, 52)]


def donor_photos():
    return [(AR.smooth_photo(70, 60, 5) * 0.6 + 50).astype(np.uint8), (255 - AR.smooth_photo(64, 72, 7) * 0.7).astype(np.uint8)]


def morphed(world, **kw):
    c = tracked(world)
    det = world['det']
    if 'dl' not in c:
        c['donors'] = donor_photos()
        c['dl'] = det.landmarks(c['donors'], DONOR_BOXES).clone()
    return det.morph_clip(c['frames'], FACES, c['donors'], donor_boxes=DONOR_BOXES, donor_landmarks=c['dl'], **dict(c['kw'], **kw))


def test_without_a_gate_the_new_kernel_is_never_reached(world, monkeypatch):
    from imm_amd import ops as _ops
    c = tracked(world)
    det = world['det']
    cm = morphed(world)

    def unreachable(*a, **k):
        raise AssertionError('landmark_scores was called without a gate')
    monkeypatch.setattr(_ops, 'landmark_scores', unreachable)
    tr = det.track(c['frames'], FACES, **c['kw'])
    same_track(tr, c['plain'], 'track() without a gate', scores=False)
    same_track(tr, c['open_ref'], 'track() without a gate against the loop', scores=False)
    again = morphed(world)
    for t in range(T):
        assert torch.equal(again.frames[t], cm.frames[t])
    same_track(again.track, c['plain'], 'morph_clip() without a gate', scores=False)
    assert again.track.qflags is None and not again.track.unsure.any()
    with pytest.raises(AssertionError, match='without a gate'):
        det.tracker(gate=c['gate'], **c['kw']).track(c['frames'], FACES)


def test_clip_morph_leaves_a_blanked_face_alone(world):
    c = tracked(world)
    frames, ref = c['frames'], c['gated_ref']
    cm = morphed(world, gate=c['gate'])
    same_track(cm.track, ref, 'the clip\'s track')
    unsure = host(cm.track.unsure)
    assert np.array_equal(unsure, ref['qflags'] != 0)
    boxes = ref['boxes']
    own = host(cm.own)

    def only(t, f):
        """The pixels of frame t inside face f's box and outside the other faces' boxes."""
        h, w = frames[t].shape[:2]
        yy, xx = np.mgrid[0:h, 0:w]
        inside = lambda b: (yy >= b[0]) & (yy < b[2]) & (xx >= b[1]) & (xx < b[3])
        m = inside(boxes[t, f])
        for g in range(len(FACES)):
            if g != f:
                m &= ~inside(boxes[t, g])
        return m
    checked = 0
    for f in range(len(FACES)):
        gone = [t for t in range(1, T) if unsure[t, f]]
        kept = [t for t in range(T) if t == 0 or not unsure[t, f]]               # frame 0 is never blanked
        for t in gone:
            m = only(t, f)
            assert m.sum() > 100, 'the test looks at a region'
            assert np.array_equal(host(cm.frames[t])[m], frames[t][m]), 'frame %d, face %d: blanked, yet its box was changed' % (t, f)
            assert np.isnan(own[t, f]).all()
            checked += 1
        if gone:
            for t in kept:
                m = only(t, f)
                assert (host(cm.frames[t])[m] != frames[t][m]).any(), 'frame %d, face %d: kept, yet its box was not pasted' % (t, f)
    assert checked >= 1


# ----------------------------------------------------------------------------------------------------------------------------
# 7. the scripts
# ----------------------------------------------------------------------------------------------------------------------------
def test_detect_script_with_quality_and_gate(ops, world, tmp_path, capsys):
    from PIL import Image
    from imm_amd.inference import LandmarkDetector
    from imm_amd.quality import QualityGate
    from imm_amd.utils.config import load_configs
    c = tracked(world)
    cfg, model, eng, P, St = D.make_model(10, 128, 2)
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, ckpt)
    imdir = tmp_path / 'clip'
    imdir.mkdir()
    frames = c['frames']
    for i, im in enumerate(frames):
        Image.fromarray(im).save(imdir / ('%03d.png' % i))
    with open(str(tmp_path / 'first.csv'), 'w') as f:
        f.write('file,y0,x0,y1,x1\n' + ''.join('000.png,%d,%d,%d,%d\n' % b[1:] for b in FACES))
    conf = D._write_config(tmp_path, str(tmp_path), str(tmp_path / 'logs'))
    tpl_path, gate_path, out = str(tmp_path / 'template.npz'), str(tmp_path / 'gate.npz'), str(tmp_path / 'out.npz')
    world['tpl'].save(tpl_path)
    det = LandmarkDetector.from_checkpoint(load_configs([conf]).model, ckpt, max_batch=4, device=DEV)
    base = ['--configs', conf, '--checkpoint', ckpt, '--images-dir', str(imdir), '--out', out, '--batch-size', '4']
    script = os.path.join(ROOT, 'scripts', 'detect.py')
    # --quality --template
    D._run_script(script, base + ['--quality', '--template', tpl_path])
    assert 'quality: mean spread' in capsys.readouterr().out
    r = np.load(out)
    q = det.quality(frames, template=world['tpl']).cpu()
    SR.same(r['spread'], q.spread.numpy(), 'script spread')
    SR.same(r['score'], q.score.numpy(), 'script score')
    SR.same(r['quality_flags'], q.flags.numpy(), 'script quality_flags')
    SR.same_bits(r['mu'], q.mu.numpy(), 'script mu')
    assert (r['score'][:, 1] > 0).all()
    # --track --gate: a gate fitted on the clip's own first pass, loose enough to blank some frames and keep others
    tr0 = det.tracker(box_smooth=0.75, fps=30.0, gate=QualityGate()).track(frames, FACES).cpu()
    sb = np.sort(tr0.score[1:, :, 0].numpy().ravel().astype(np.float64))
    gate = QualityGate(max_spread=float((sb[len(sb) // 2 - 1] + sb[len(sb) // 2]) / 2), K=10, S=128, heatmap=16)
    gate.save(gate_path)
    D._run_script(script, base + ['--track', '--boxes', str(tmp_path / 'first.csv'), '--fps', '30', '--box-smooth', '0.75', '--gate', gate_path])
    tr = det.tracker(box_smooth=0.75, fps=30.0, gate=QualityGate.load(gate_path, detector=det)).track(frames, FACES).cpu()
    said = capsys.readouterr().out
    assert '6 frames, 3 faces tracked' in said and '%d lost, %d unsure)' % (int(tr.lost.sum()), int(tr.unsure.sum())) in said
    r = np.load(out)
    for k in FIELDS + ('spread', 'score'):
        SR.same(r[k], getattr(tr, k).numpy(), 'script ' + k)
    SR.same(r['quality_flags'], tr.qflags.numpy(), 'script quality_flags')
    assert int(tr.unsure.sum()) == int((r['quality_flags'] != 0).sum())


def test_test_script_fits_a_gate_on_the_test_split(ops, tmp_path, capsys):
    from dataset_fixtures import make_celeba_tree
    from imm_amd.alignment import LandmarkTemplate
    from imm_amd.inference import LandmarkDetector
    from imm_amd.quality import QualityGate
    from imm_amd.utils.config import load_configs
    from imm_amd.utils.dataset_import import import_dataset
    root = str(tmp_path / 'celeba')
    make_celeba_tree(root, n=40)
    cfg, model, eng, P, St = D.make_model(3, 128, 4)
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, ckpt)
    conf = D._write_config(tmp_path, root, str(tmp_path / 'logs'), n_maps=3)
    tplp, gatep = str(tmp_path / 'template.npz'), str(tmp_path / 'gate.npz')
    LandmarkTemplate(np.array([[-0.5, -0.4], [0.3, 0.6], [0.5, -0.2]]), 128).save(tplp)
    script = os.path.join(ROOT, 'scripts', 'test.py')
    base = ['--configs', conf, '--train-dataset', 'mafl', '--test-dataset', 'mafl', '--checkpoint', ckpt, '--batch-size', '4', '--detector']
    with pytest.raises(ValueError, match='go together'):
        D._run_script(script, base + ['--save-gate', gatep, '--gate-quantile', '0.9'])
    D._run_script(script, base + ['--save-gate', gatep, '--gate-quantile', '0.9', '--gate-margin', '1.25', '--template', tplp])
    assert 'quality gate of' in capsys.readouterr().out
    det = LandmarkDetector.from_checkpoint(load_configs([conf]).model, ckpt, max_batch=4, device=DEV)
    gate = QualityGate.load(gatep, detector=det)
    assert (gate.K, gate.S, gate.heatmap) == (3, 128, 16)
    test = import_dataset('celeba')(root, dataset='mafl', subset='test', order_stream=True, tps=False, image_size=[128, 128])
    tpl = LandmarkTemplate.load(tplp)
    score = np.concatenate([det.quality(b['future_image'], template=tpl).cpu().score.numpy()
                            for b in test.get_dataset(4, repeat=False, shuffle=False, device=DEV)]).astype(np.float64)
    assert gate.max_spread == 1.25 * float(np.quantile(score[:, 0], 0.9)) and gate.max_residual == 1.25 * float(np.quantile(score[:, 1], 0.9))
    # a gate fitted on these faces passes at least the quantile of them
    q = np.concatenate([det.quality(b['future_image'], template=tpl, gate=gate).cpu().flags.numpy()
                        for b in test.get_dataset(4, repeat=False, shuffle=False, device=DEV)])
    assert ((q & 1) == 0).mean() >= 0.9 and ((q & 2) == 0).mean() >= 0.9
