"""Re-enactment on the MI355X: imm_retarget in guarded buffers against the numpy restatement of include/imm_retarget.h
(tests/retarget_reference.py) bit for bit, ImageGenerator.reenact against the loop over public calls it replaces (track(), .cpu(), the
restatement, repose() per frame), its identities, its side effects, and the script.

"Bit for bit" compares the stored bits of every element; two NaNs count as equal whatever their payloads (same_bits of
tests/test_track_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alignment_reference as AR                  # noqa: E402
import guarded                                    # noqa: E402
import retarget_reference as R                    # noqa: E402
import test_detector_gpu as D                     # noqa: E402  (make_model, images, _run_script, _write_config)
import test_track_gpu as TT                       # noqa: E402  (same_bits, same_track, clip)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
same_bits = TT.same_bits
F32, F64 = np.float32, np.float64


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


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the restatement
# ----------------------------------------------------------------------------------------------------------------------------
NAN_FACE, COINCIDENT_FACE, CLAMP_FACE = 1, 2, 0
LOST_FRAME = 2


def kernel_case(n, K, seed):
    """Four frames of one driver and n source faces: the driver's shape drifts, turns, grows and changes (noise) from frame to frame
    and is lost on frame 2 (every face held, released on frame 3); with n >= 3 face 1 has a NaN landmark and face 2 coincident
    landmarks (held throughout), and face 0 has the driver's own shape at one and a half times its box, so that in either motion
    some of its landmarks lie or are carried across the border of the box (the clamp).
    Returns (q f32 [4, K, 2], driver flags [4], m f32 [n, K, 2], the faces held on every frame)."""
    rng = np.random.RandomState(seed)
    shape = rng.uniform(-60.0, 60.0, size=(K, 2))
    shape[0] = [55.0, -50.0]
    qs = []
    for t in range(4):
        ang, sc, sh = 0.12 * t, 1.0 + 0.08 * t, np.array([150.0 + 9.0 * t, 170.0 - 7.0 * t])
        rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]) * sc
        qs.append((shape @ rot.T + sh + (rng.standard_normal((K, 2)) * 2.0 if t else 0.0)).astype(F32))
    dflags = [0, 2, 1, 0]                                    # outside alone (bit 1) holds nothing; lost (bit 0) on frame 2
    m = rng.uniform(-0.6, 0.6, size=(n, K, 2)).astype(F32)
    always = []
    if n >= 3:
        m[CLAMP_FACE] = (shape / 40.0).astype(F32)
        m[NAN_FACE, K // 2, 1] = np.nan
        m[COINCIDENT_FACE] = m[COINCIDENT_FACE, :1]
        always = [NAN_FACE, COINCIDENT_FACE]
    if n >= 65:
        m[64, 0, 0] = np.inf                                 # a face of the second block, held throughout
        always.append(64)
    return np.stack(qs), dflags, m, always


def settings(n, K):
    """(relative, rigid, gain): both motions and both rigid values across the parametrisation, gain 1 and 0.5."""
    return K != 10, n != 3, 0.5 if K == 64 else 1.0


def run_kernel_case(ops, n, K, seed, alias):
    qs, dflags, m, always = kernel_case(n, K, seed)
    relative, rigid, gain = settings(n, K)
    anchor_ref = np.full((K, 2), np.nan)
    anchor = guarded.out((K, 2), torch.float64, DEV)          # NaN body: init writes every value and reads none
    m_d = guarded.inp(torch.from_numpy(m), DEV)
    pose = guarded.out((n, K, 2), torch.float32, DEV, fill=torch.from_numpy(m)) if alias else None
    prev = m
    for t in range(4):
        q_d = guarded.inp(torch.from_numpy(qs[t]), DEV)
        fl_d = guarded.inp(torch.tensor([dflags[t]], dtype=torch.int32), DEV)
        flags = guarded.out((n,), torch.int32, DEV)
        if alias:
            prev_d = out = pose
        else:
            prev_d = guarded.inp(torch.from_numpy(prev), DEV)
            out = guarded.out((n, K, 2), torch.float32, DEV)
        ops.retarget(q_d, anchor, fl_d, m_d, prev_d, int(t == 0), relative, rigid, gain, out, flags)
        torch.cuda.synchronize()
        r_out, r_flags = R.retarget(qs[t], anchor_ref, dflags[t], m, prev, int(t == 0), relative, rigid, gain)
        what = 'n=%d K=%d frame %d ' % (n, K, t)
        same_bits(out, r_out, what + 'out')
        same_bits(flags, r_flags, what + 'flags')
        same_bits(anchor, anchor_ref, what + 'anchor')
        assert np.array_equal(anchor_ref, qs[0].astype(F64)), 'the anchor is the first frame\'s points, set once'
        # the case holds what it says it holds: exactly the named faces are held, every other face's pose moved
        want = np.zeros(n, dtype=bool)
        want[always] = True
        if t == LOST_FRAME:
            want[:] = True
        assert np.array_equal(r_flags != 0, want), (what, r_flags.tolist())
        assert np.array_equal(r_out[want].view(np.int32), prev[want].view(np.int32))
        if t > 0 or not relative:                              # a still first frame in relative mode is the face's own pose: out == m
            for i in np.nonzero(~want)[0]:
                assert not np.array_equal(r_out[i], prev[i]), (what, i)
        elif rigid:
            same_bits(r_out[~want], np.clip(m[~want], -1.0, 1.0), what + 'a still clip is m (inside its box)')
        assert (np.abs(r_out[~want]) <= 1.0).all()
        if n >= 3 and not want[CLAMP_FACE]:
            hit = np.abs(r_out[CLAMP_FACE]) == 1.0
            assert hit.any() and not hit.all(), 'some landmarks of the clamp face end on the border of its box, not all'
        prev = r_out


@pytest.mark.parametrize('K', [3, 10, 64])
@pytest.mark.parametrize('n', [1, 3, 65])
def test_retarget_equals_the_restatement(ops, n, K):
    run_kernel_case(ops, n, K, 100 * n + K, alias=False)


def test_retarget_may_write_the_poses_it_holds(ops):
    """out may be the buffer `prev`: a thread reads its row before it writes it."""
    run_kernel_case(ops, 65, 5, 9, alias=True)


def test_ops_retarget_checks_its_tensors(ops):
    K, n = 4, 2
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    good = dict(q=z(K, 2), anchor=z(K, 2, dt=torch.float64), driver_flags=z(1, dt=torch.int32), m=z(n, K, 2), prev=z(n, K, 2),
                out=z(n, K, 2), flags=z(n, dt=torch.int32))
    for name, bad in (('q', z(K, 3)), ('anchor', z(K, 2)), ('driver_flags', z(2, dt=torch.int32)), ('prev', z(n + 1, K, 2)),
                      ('out', z(n, K, 2, dt=torch.float64)), ('flags', z(n)), ('q', z(2, K).t())):
        a = dict(good, **{name: bad})
        with pytest.raises(ValueError, match=name):
            ops.retarget(a['q'], a['anchor'], a['driver_flags'], a['m'], a['prev'], 1, True, True, 1.0, a['out'], a['flags'])


# ----------------------------------------------------------------------------------------------------------------------------
# 2. reenact() against the loop over public calls
# ----------------------------------------------------------------------------------------------------------------------------
T = TT.T
PHOTO_SIZES = [(120, 100), (96, 110)]
BOXES = [(0, 10, 8, 90, 80), (1, 20, 30, 80, 100), (0, -12, 30, 60, 95)]              # the third reaches outside its photo
FOURTH = (1, 4, 6, 70, 64)
DRIVER = (10, 8, 70, 60)
BETA, OE, FPS = 0.5, TT.OE, TT.FPS
FEATHER = 0.125


def photos():
    return [AR.smooth_photo(h, w, 40 + i) for i, (h, w) in enumerate(PHOTO_SIZES)]


def the_loop(gen, ims, frames, boxes, relative=True, rigid=True, gain=1.0, smooth=True):
    """What a user does at the parent commit: track(), .cpu(), the rule on the host, repose() per frame."""
    from imm_amd.tracking import OneEuro
    tr = gen.detector.track(frames, [DRIVER], box_smooth=BETA, one_euro=OneEuro(*OE), fps=FPS).cpu()
    m = gen.detector.landmarks(ims, boxes).cpu().numpy()
    pts = (tr.points_smooth if smooth else tr.points)[:, 0].numpy()
    lm, flags = R.retarget_clip(pts, tr.flags[:, 0].numpy(), m, relative, rigid, gain)
    out, faces = [], []
    for t in range(len(frames)):
        o, f, _lm = gen.repose(ims, torch.from_numpy(lm[t]), boxes, feather=FEATHER, return_faces=True)
        out.append([x.cpu().numpy() for x in o])
        faces.append(f.cpu().numpy())
    return {'track': tr, 'm': m, 'landmarks': lm, 'flags': flags, 'frames': out, 'faces': np.stack(faces)}


def kwargs(**kw):
    from imm_amd.tracking import OneEuro
    base = dict(box_smooth=BETA, one_euro=OneEuro(*OE), fps=FPS, feather=FEATHER, return_faces=True)
    base.update(kw)
    return base


@pytest.fixture(scope='module')
def world(ops):
    """One model and generator (K = 10, S = 128, max_batch 4), the photos, the clip, and the user's loop run once."""
    cfg, model, eng, P, St = D.make_model(10, 128, 2)
    gen = model.image_generator(128, max_batch=4)
    ims, frames = photos(), TT.clip()
    return gen, eng, ims, frames, the_loop(gen, ims, frames, BOXES)


def same_result(r, ref, what, faces=slice(None), n_photos=2):
    same_bits(r.landmarks[:, faces], ref['landmarks'], what + ' landmarks')
    same_bits(r.flags[:, faces], ref['flags'], what + ' flags')
    if ref.get('faces') is not None:
        same_bits(r.faces[:, faces], ref['faces'], what + ' faces')
    if ref.get('frames') is not None:
        assert len(r.frames) == len(ref['frames'])
        for t, (got, want) in enumerate(zip(r.frames, ref['frames'])):
            assert len(got) == len(want) == n_photos
            for i, (g, w) in enumerate(zip(got, want)):
                assert g.dtype == torch.uint8 and g.is_cuda
                same_bits(g, w, '%s frame %d photo %d' % (what, t, i))


def test_reenact_equals_the_loop_over_public_calls(world):
    from imm_amd.reenact import Reenactment
    from imm_amd.tracking import Track
    gen, eng, ims, frames, ref = world
    r = gen.reenact(ims, frames, DRIVER, BOXES, **kwargs())
    torch.cuda.synchronize()
    assert isinstance(r, Reenactment) and len(r) == T and isinstance(r.track, Track)
    assert tuple(r.landmarks.shape) == (T, 3, 10, 2) and r.landmarks.is_cuda and r.landmarks.dtype == torch.float32
    assert tuple(r.flags.shape) == (T, 3) and r.flags.dtype == torch.int32 and r.held.dtype == torch.bool and not bool(r.held.any())
    assert tuple(r.faces.shape) == (T, 3, 128, 128, 3)
    same_result(r, ref, 'reenact')
    TT.same_track(r.track, ref['track'], 'the driver\'s track')
    for t in range(T):
        for i, im in enumerate(ims):
            assert tuple(r.frames[t][i].shape) == im.shape
    base = r.frames[0][0].untyped_storage().data_ptr()
    assert all(f.untyped_storage().data_ptr() == base for fr in r.frames for f in fr), 'views of one buffer'
    # the case moves: a still first frame is the faces' own poses, every later frame another pose, every frame another picture than the photo
    lm = ref['landmarks']
    same_bits(lm[0], ref['m'], 'frame 0 is m')
    assert all(np.abs(lm[t] - lm[t - 1]).max() > 1e-4 for t in range(1, T))
    print('\nREENACT max |landmarks[t] - m| per frame: %s' % [float(np.abs(lm[t] - ref['m']).max()) for t in range(T)])
    for t in range(T):
        for i, im in enumerate(ims):
            assert (ref['frames'][t][i] != im).mean() > 0.2
    # a pose that moves by a hundredth of a 16 x 16 map cell need not change a 16-bit Gaussian map, let alone a u8 frame: whether the
    # pictures change from frame to frame is printed, not asserted
    print('REENACT faces that differ from the frame before: %s' % [bool((ref['faces'][t] != ref['faces'][t - 1]).any()) for t in range(1, T)])
    assert all(np.array_equal(im, p) for im, p in zip(ims, photos())), 'the photos are not written'
    # the other motion, without head motion, half the gain
    ref2 = the_loop(gen, ims, frames, BOXES, relative=False, rigid=False, gain=0.5)
    r2 = gen.reenact(ims, frames, [DRIVER], BOXES, motion='absolute', rigid=False, gain=0.5, **kwargs())
    same_result(r2, ref2, 'absolute, rigid=False, gain 0.5')
    assert np.abs(ref2['landmarks'] - ref['landmarks']).max() > 1e-3


def test_identities(world):
    gen, eng, ims, frames, ref = world
    # a still clip, and gain = 0: every frame is repose() at the faces' own landmarks
    m = gen.detector.landmarks(ims, BOXES)
    own, own_faces, _ = gen.repose(ims, m, BOXES, feather=FEATHER, return_faces=True)
    own_ref = {'landmarks': np.stack([m.cpu().numpy()] * T), 'flags': np.zeros((T, 3), np.int32),
               'faces': np.stack([own_faces.cpu().numpy()] * T), 'frames': [[o.cpu().numpy() for o in own]] * T}
    still = gen.reenact(ims, [frames[0]] * T, DRIVER, BOXES, **kwargs())
    same_result(still, own_ref, 'a clip of identical frames')
    same_result(gen.reenact(ims, frames, DRIVER, BOXES, gain=0.0, **kwargs()), own_ref, 'gain=0')
    # chunks and a second run
    same_result(gen.reenact(ims, frames, DRIVER, BOXES, chunk_frames=1, **kwargs()), ref, 'chunk_frames=1')
    same_result(gen.reenact(ims, frames, DRIVER, BOXES, chunk_frames=2, **kwargs()), ref, 'chunk_frames=2')
    same_result(gen.reenact(ims, frames, DRIVER, BOXES, **kwargs()), ref, 'a second run')
    # smooth=False reads the raw points: the same first frame (the filter passes it through), other poses after it
    raw = gen.reenact(ims, frames, DRIVER, BOXES, smooth=False, **kwargs())
    same_result(raw, the_loop(gen, ims, frames, BOXES, smooth=False), 'smooth=False')
    same_bits(raw.landmarks[0], ref['landmarks'][0], 'smooth=False frame 0')
    assert all((raw.landmarks[t].cpu().numpy() != ref['landmarks'][t]).any() for t in range(1, T))
    # paste=False: no frames, the same faces
    bare = gen.reenact(ims, frames, DRIVER, BOXES, paste=False, **kwargs())
    assert bare.frames is None
    same_result(bare, dict(ref, frames=None), 'paste=False')
    quiet = gen.reenact(ims, frames, DRIVER, BOXES, **kwargs(return_faces=False))
    assert quiet.faces is None
    same_result(quiet, dict(ref, faces=None), 'return_faces=False')
    # a fourth source face in the same bucket leaves the first three as they are (its paste may cover their pixels: the faces decide)
    more = gen.reenact(ims, frames, DRIVER, BOXES + [FOURTH], **kwargs())
    assert tuple(more.landmarks.shape) == (T, 4, 10, 2)
    same_result(more, dict(ref, frames=None), 'with a fourth face', faces=slice(0, 3))
    assert (more.landmarks[1:, 3] != more.landmarks[:-1, 3]).any()
    # refusals reach the user before anything runs
    with pytest.raises(ValueError, match='max_batch'):
        gen.reenact(ims, frames, DRIVER, BOXES + [FOURTH] * 2)
    with pytest.raises(ValueError, match='ONE driving face'):
        gen.reenact(ims, frames, [DRIVER, DRIVER], BOXES)
    with pytest.raises(NotImplementedError, match='template'):
        gen.reenact(ims, frames, DRIVER, BOXES, template=object())


def test_reenact_has_no_side_effects(world):
    gen, eng, ims, frames, ref = world
    x, y = D.images(3, 128, 21), D.images(3, 128, 22)
    lm = torch.from_numpy(np.random.RandomState(5).uniform(-0.6, 0.6, size=(3, 10, 2)).astype(F32))

    def probe():
        out = [gen.detector.detect(x).cpu(), gen.reconstruct(x, y).cpu()] + [o.cpu() for o in gen.repose(ims, lm, BOXES)]
        torch.cuda.synchronize()
        return out
    before = probe()
    model_before = (eng.named_parameters(), eng.named_state(), eng.loss_agg.clone(), eng.step_count.clone())
    gen.reenact(ims, frames, DRIVER, BOXES, motion='absolute', rigid=False)
    after = probe()
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))
    model_after = (eng.named_parameters(), eng.named_state(), eng.loss_agg.clone(), eng.step_count.clone())
    for a, b in zip(model_before[:2], model_after[:2]):
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(model_before[2], model_after[2]) and torch.equal(model_before[3], model_after[3])


# ----------------------------------------------------------------------------------------------------------------------------
# 3. the script
# ----------------------------------------------------------------------------------------------------------------------------
def test_generate_script_reenacts(ops, tmp_path, capsys):
    from PIL import Image
    from imm_amd.generation import ImageGenerator
    from imm_amd.utils.config import load_configs
    cfg, model, eng, P, St = D.make_model(10, 128, 2)
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, ckpt)
    ims, frames = photos(), TT.clip()
    (tmp_path / 'photos').mkdir()
    (tmp_path / 'clip').mkdir()
    for i, im in enumerate(ims):
        Image.fromarray(im).save(tmp_path / 'photos' / ('p%d.png' % i))
    for i, im in enumerate(frames):
        Image.fromarray(im).save(tmp_path / 'clip' / ('%03d.png' % i))
    with open(str(tmp_path / 'faces.csv'), 'w') as f:
        f.write('file,y0,x0,y1,x1\n' + ''.join('p%d.png,%d,%d,%d,%d\n' % b for b in BOXES))
    conf = D._write_config(tmp_path, str(tmp_path), str(tmp_path / 'logs'))
    out_dir, npz = str(tmp_path / 'out'), str(tmp_path / 'out.npz')
    D._run_script(os.path.join(ROOT, 'scripts', 'generate.py'), [
        '--configs', conf, '--checkpoint', ckpt, '--appearance-dir', str(tmp_path / 'photos'), '--boxes', str(tmp_path / 'faces.csv'),
        '--drive-dir', str(tmp_path / 'clip'), '--drive-box', '%d,%d,%d,%d' % DRIVER, '--out-dir', out_dir, '--npz', npz, '--batch-size', '4',
        '--motion', 'absolute', '--no-rigid', '--gain', '0.75', '--fps', '30', '--feather', '0.25'])
    assert '5 frames, 3 faces re-enacted' in capsys.readouterr().out
    gen = ImageGenerator.from_checkpoint(load_configs([conf]).model, ckpt, max_batch=4, device=DEV)
    r = gen.reenact(ims, frames, DRIVER, BOXES, motion='absolute', rigid=False, gain=0.75, fps=30.0, feather=0.25)
    saved = np.load(npz)
    same_bits(saved['landmarks'], r.landmarks.cpu().numpy(), 'script landmarks')
    same_bits(saved['flags'], r.flags.cpu().numpy(), 'script flags')
    assert list(saved['frames']) == ['%03d.png' % t for t in range(T)] and list(saved['appearance']) == ['p0.png', 'p1.png']
    assert sorted(os.listdir(out_dir)) == ['%03d' % t for t in range(T)]
    for t in range(T):
        assert sorted(os.listdir(os.path.join(out_dir, '%03d' % t))) == ['p0.png', 'p1.png']
        for i in range(2):
            png = np.asarray(Image.open(os.path.join(out_dir, '%03d' % t, 'p%d.png' % i)))
            same_bits(r.frames[t][i], png, 'script frame %d photo %d' % (t, i))
    assert (r.landmarks[1] != r.landmarks[0]).any()
