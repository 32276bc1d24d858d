"""Re-enactment, host side (no GPU): the ABI of imm_retarget and its argument validation, hand-derived known answers of the numpy
restatement of the rule (tests/retarget_reference.py), and the refusals of plan_reenact."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retarget_reference as R                                              # noqa: E402

from imm_amd import reenact as RE                                           # noqa: E402  (imports without a GPU)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
# the driver's first frame, K = 3: mean (130, 220), u = q0 - mean, sum |u|^2 = 4200
Q0 = np.array([[100.0, 200.0], [160.0, 200.0], [130.0, 260.0]])
U = np.array([[-30.0, -20.0], [30.0, -20.0], [0.0, 40.0]])
MM = np.array([0.125, -0.25])
M = (U / 64.0 + MM).astype(F32)                                             # a = (1 / 64, 0): every value exact in binary
M_TURNED = (np.stack([-U[:, 1], U[:, 0]], axis=1) / 64.0 + MM).astype(F32)  # z -> i z / 64 with z = y + ix: a = (0, 1 / 64)
PREV = np.array([[0.5, 0.25], [-0.5, 0.75], [0.0, -0.125]], dtype=F32)


def face(q, m=M, q0=Q0, driver_flags=0, prev=PREV, relative=True, rigid=True, gain=1.0):
    return R.retarget_face(np.asarray(q, F32), np.asarray(q0, F64), driver_flags, m, prev, relative, rigid, gain)


def bits(a):
    return np.asarray(a, dtype=F32).view(np.int32)


# ----------------------------------------------------------------------------------------------------------------------------
# ABI and validation
# ----------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_retarget_entry_point():
    from imm_amd import _lib as L
    assert L.ABI_VERSION >= 29
    header = open(os.path.join(ROOT, 'include', 'imm_retarget.h')).read()
    assert L.symbols('imm_retarget.h') == ['imm_retarget']
    assert L.symbols('imm_track.h') == ['imm_track_step'], 'imm_track.h keeps its one symbol'
    for text in ('THE RULE', 'rounded separately', 'fit(z, p)', 'HELD', 'rigid == 0', 'relative', 'absolute', 'den_a == 0', 'nb'):
        assert text in header, text
    src = open(os.path.join(ROOT, 'imm_amd', 'csrc', 'retarget.hip')).read()
    assert 'fp contract(off)' in src and not re.search(r'\b(sin|cos|exp|log|pow|atan2?|tan|sqrt)f?\s*\(', src), 'only + - * / fabs fmin fmax isfinite'


def test_retarget_validates_its_arguments_without_a_device():
    from imm_amd import _lib as L
    lib = L.load()
    one = C.c_void_p(16)                                   # a non-null pointer that is never read: validation comes first
    #       q    anchor dflags m   prev  K  n  init rel rigid gain out  flags stream
    good = [one, one, one, one, one, 10, 3, 0, 1, 1, 1.0, one, one, None]
    nan, inf = float('nan'), float('inf')
    bad_args = [(i, None) for i in (0, 1, 2, 3, 4, 11, 12)]                                              # null pointers
    bad_args += [(5, 0), (5, 65), (5, -1), (6, 0), (6, 65536), (6, -1)]                                  # K, n
    bad_args += [(7, 2), (7, -1), (8, 2), (8, -1), (9, 2), (9, -1)]                                      # init, relative, rigid
    bad_args += [(10, nan), (10, -1.0), (10, 5.0), (10, inf), (10, -inf), (10, 4.000001)]                # gain
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert lib.imm_retarget(*args) == -1, (i, bad)
        assert b'retarget' in lib.imm_last_error()


# ----------------------------------------------------------------------------------------------------------------------------
# known answers, K = 3
# ----------------------------------------------------------------------------------------------------------------------------
def test_the_fit_of_the_fixture():
    a_r, a_i, mz0, mz1, mp0, mp1, den = R.fit(Q0, M.astype(F64))
    assert (a_r, a_i, mz0, mz1, mp0, mp1, den) == (0.015625, 0.0, 130.0, 220.0, 0.125, -0.25, 4200.0)
    a_r, a_i = R.fit(Q0, M_TURNED.astype(F64))[:2]
    assert (a_r, a_i) == (0.0, 0.015625)


@pytest.mark.parametrize('rigid', [True, False])
def test_a_still_clip_gives_the_own_landmarks_bit_for_bit(rigid):
    rng = np.random.RandomState(3)
    for m in (M, M_TURNED, rng.uniform(-0.9, 0.9, (3, 2)).astype(F32)):
        for gain in (1.0, 0.5, 4.0):
            out, fl = face(Q0, m=m, rigid=rigid, gain=gain)
            if rigid:
                assert fl == 0 and out.dtype == F32 and np.array_equal(bits(out), bits(m))
            else:
                assert fl == 0 and np.abs(out - m).max() < 1e-6               # b = 1 exactly here, the division leaves q0 exactly
                assert np.array_equal(bits(out), bits(m))
    q0 = rng.uniform(50, 300, (10, 2)).astype(F32)                           # and with no round number anywhere
    m = rng.uniform(-0.9, 0.9, (10, 2)).astype(F32)
    out, fl = R.retarget_face(q0, q0.astype(F64), 0, m, m, True, True, 1.0)
    assert fl == 0 and np.array_equal(bits(out), bits(m))


def test_a_ten_pixel_shift_moves_the_face_by_gain_times_a_times_ten():
    for gain in (1.0, 0.5, 2.0):
        out, fl = face(Q0 + [10.0, 0.0], gain=gain)
        assert fl == 0 and np.array_equal(out, (M.astype(F64) + [gain * 10.0 / 64.0, 0.0]).astype(F32))          # a = (1 / 64, 0)
        out, fl = face(Q0 + [10.0, 0.0], m=M_TURNED, gain=gain)
        assert fl == 0 and np.array_equal(out, (M_TURNED.astype(F64) + [0.0, gain * 10.0 / 64.0]).astype(F32))   # a = (0, 1 / 64): a turn
    out, _ = face(Q0 + [0.0, -4.0])
    assert np.array_equal(out, (M.astype(F64) + [0.0, -0.0625]).astype(F32))
    # rigid=False takes the whole shift for head motion
    out, fl = face(Q0 + [10.0, 0.0], rigid=False)
    assert fl == 0 and np.array_equal(bits(out), bits(M))


def test_a_turned_and_grown_driver_leaves_the_face_alone_without_head_motion():
    turned = np.array([300.0, 100.0]) + np.stack([-2.0 * U[:, 1], 2.0 * U[:, 0]], axis=1)        # b = (0, 2): a quarter turn, twice the size
    for m in (M, M_TURNED):
        out, fl = face(turned, m=m, rigid=False)
        assert fl == 0 and np.array_equal(bits(out), bits(m))
        out, fl = face(turned, m=m, rigid=True)
        assert fl == 0 and not np.array_equal(out, m), 'with rigid=True the head motion moves the face'
    # one displaced landmark on top of that head motion: what the similarity does not absorb moves the face, and as the residual of a
    # least-squares fit about the means it sums to zero over the points (with K = 3 the fit absorbs much of one point's displacement)
    moved = turned.copy()
    moved[2] += [0.0, 12.0]
    out, fl = face(moved, rigid=False)
    d = out.astype(F64) - M
    assert fl == 0 and np.abs(d).max() > 0.02 and np.abs(d.sum(axis=0)).max() < 1e-6


def test_absolute_mode_lays_the_fitted_driver_shape_over_the_face():
    out, fl = face(Q0, relative=False)
    assert fl == 0 and np.array_equal(bits(out), bits(M)), 'm is an exact similarity of q0: the fit returns it'
    m = M.copy()
    m[1] += F32(0.1)                                                          # no similarity of q0 any more
    out, fl = face(Q0, m=m, relative=False)
    z, p = Q0[:, 0] + 1j * Q0[:, 1], m[:, 0].astype(F64) + 1j * m[:, 1].astype(F64)
    a = (np.conj(z - z.mean()) * (p - p.mean())).sum() / (np.abs(z - z.mean()) ** 2).sum()
    want = p.mean() + a * (z - z.mean())
    assert fl == 0 and np.abs(out[:, 0] - want.real).max() < 1e-6 and np.abs(out[:, 1] - want.imag).max() < 1e-6
    assert np.abs(out - m).max() > 0.01
    # gain = 0 is the face's own pose in both modes
    for relative in (True, False):
        out, fl = face(Q0 + [7.0, 3.0], m=m, relative=relative, gain=0.0)
        assert fl == 0 and np.array_equal(bits(out), bits(m))


def test_each_cause_of_a_held_pose_returns_prev():
    moved = Q0 + [10.0, 0.0]
    out, fl = face(moved)
    assert fl == 0 and not np.array_equal(out, PREV)
    cases = {'the driver is lost': dict(q=moved, driver_flags=1), 'lost and outside': dict(q=moved, driver_flags=3)}
    for name, bad in (('NaN', np.nan), ('inf', np.inf), ('-inf', -np.inf)):
        q = moved.copy()
        q[1, 0] = bad
        cases['q ' + name] = dict(q=q)
        q0 = Q0.copy()
        q0[2, 1] = bad
        cases['q0 ' + name] = dict(q=moved, q0=q0)
        m = M.copy()
        m[0, 1] = bad
        cases['m ' + name] = dict(q=moved, m=m)
    cases['den_a == 0: the anchor points coincide'] = dict(q=moved, q0=np.tile([[130.0, 220.0]], (3, 1)))
    cases['na == 0: the own landmarks coincide'] = dict(q=moved, m=np.tile(np.array([[0.25, -0.5]], F32), (3, 1)))
    cases['a value that is not finite'] = dict(q=moved, q0=Q0 * 1e298, m=(M * F32(1e38)).astype(F32))
    for name, kw in cases.items():
        for rigid in (True, False):
            for relative in (True, False):
                out, fl = face(rigid=rigid, relative=relative, **kw)
                assert fl == R.HELD == RE.FLAG_HELD and np.array_equal(bits(out), bits(PREV)), (name, rigid, relative)
    assert np.isfinite(Q0 * 1e298).all() and np.isfinite(M * F32(1e38)).all()
    # outside alone (bit 1 of the driver's flags) holds nothing
    assert face(moved, driver_flags=2)[1] == 0
    # rigid=False only: the current points coincide (b = 0)
    q = np.tile([[50.0, 60.0]], (3, 1))
    out, fl = face(q, rigid=False)
    assert fl == 1 and np.array_equal(bits(out), bits(PREV))
    assert face(q, rigid=True)[1] == 0
    # a held NaN of prev is copied as it is
    prev = PREV.copy()
    prev[0, 0] = np.nan
    out, fl = face(moved, driver_flags=1, prev=prev)
    assert fl == 1 and np.isnan(out[0, 0]) and np.array_equal(out[1:], prev[1:])


def test_the_clamp():
    out, fl = face(Q0 + [1000.0, -1000.0])
    assert fl == 0 and np.array_equal(out, np.tile(np.array([[1.0, -1.0]], F32), (3, 1)))
    out, fl = face(Q0 + [10.0, 0.0], gain=4.0)                               # 0.59375 + 0.625 leaves the box, the others stay inside
    assert fl == 0 and out[:, 0].tolist() == [0.28125, 1.0, 0.75]


def test_a_clip_holds_the_pose_of_the_frame_before():
    pts = np.stack([Q0, Q0 + [10.0, 0.0], Q0 + [20.0, 0.0], Q0 + [30.0, 0.0]]).astype(F32)
    m = np.stack([M, M_TURNED])
    lm, fl = R.retarget_clip(pts, [0, 0, 1, 0], m)
    assert lm.shape == (4, 2, 3, 2) and lm.dtype == F32 and fl.tolist() == [[0, 0], [0, 0], [1, 1], [0, 0]]
    assert np.array_equal(lm[0], m) and np.array_equal(lm[2], lm[1]) and not np.array_equal(lm[3], lm[2])
    assert np.array_equal(lm[3, 0], (M.astype(F64) + [30.0 / 64.0, 0.0]).clip(-1, 1).astype(F32))
    anchor = np.full((3, 2), 7.0)
    R.retarget(pts[1], anchor, 0, m, m, 1)
    assert np.array_equal(anchor, pts[1].astype(F64)), 'init sets the anchor'
    R.retarget(pts[2], anchor, 0, m, m, 0)
    assert np.array_equal(anchor, pts[1].astype(F64)), 'and only init does'


# ----------------------------------------------------------------------------------------------------------------------------
# plan_reenact
# ----------------------------------------------------------------------------------------------------------------------------
def test_plan_reenact():
    import inspect
    import torch
    from imm_amd import generation as GEN
    from imm_amd import tracking as TR
    photos = [np.zeros((30, 40, 3), np.uint8), np.zeros((20, 25), np.uint8)]
    frames = [np.zeros((50, 60, 3), np.uint8), np.zeros((40, 45, 3), np.uint8)]
    p = RE.plan_reenact(photos, frames, (2, 3, 20, 30), [(0, 1, 2, 20, 30), (1, -5, -5, 10, 10), (0, 0, 0, 9, 9)], 4)
    assert p.rows.tolist() == [[0, 1, 2, 20, 30], [1, -5, -5, 10, 10], [0, 0, 0, 9, 9]] and p.rows.dtype == np.int32
    assert p.driver_row.tolist() == [[0, 2, 3, 20, 30]] and p.photos[1].shape == (20, 25, 3) and len(p.frames) == 2
    assert (p.relative, p.rigid, p.gain, p.smooth, p.feather, p.paste, p.box_smooth, p.fps, p.chunk_frames) == (
        True, True, 1.0, True, 0.125, True, 0.5, 25.0, 32)
    p = RE.plan_reenact(photos, frames, [(0, 2, 3, 20, 30)], None, 2, 'absolute', False, 0.0, False, 0.0, False, 1.0, None, 30.0, 1)
    assert p.rows.tolist() == [[0, 0, 0, 30, 40], [1, 0, 0, 20, 25]] and (p.relative, p.rigid, p.gain, p.paste, p.one_euro) == (
        False, False, 0.0, False, None)
    box = (2, 3, 20, 30)
    with pytest.raises(ValueError, match='ONE driving face'):
        RE.plan_reenact(photos, frames, [box, box], None, 4)                                 # two driver faces
    with pytest.raises(ValueError, match='ONE driving face'):
        RE.plan_reenact(photos, frames, [], None, 4)
    with pytest.raises(ValueError, match=r'frames\[0\]'):
        RE.plan_reenact(photos, frames, (1, 2, 3, 20, 30), None, 4)                          # the driver in another frame
    with pytest.raises(ValueError, match='empty'):
        RE.plan_reenact(photos, frames, (2, 3, 2, 30), None, 4)
    with pytest.raises(ValueError, match='max_batch'):
        RE.plan_reenact(photos, frames, box, [(0, 1, 2, 20, 30)] * 5, 4)                     # n > max_batch
    for tensor in (torch.zeros(2, 128, 128, 3), np.zeros((2, 30, 40, 3), np.uint8)):
        with pytest.raises(ValueError, match='list of u8'):
            RE.plan_reenact(tensor, frames, box, None, 4)                                    # a tensor batch as photos
        with pytest.raises(ValueError, match='list of u8'):
            RE.plan_reenact(photos, tensor, box, None, 4)
    with pytest.raises(ValueError, match='uint8'):
        RE.plan_reenact([np.zeros((30, 40, 3), np.float32)], frames, box, None, 4)
    with pytest.raises(ValueError, match='no frames'):
        RE.plan_reenact(photos, [], box, None, 4)
    for bad in ('tps', 'rel', None, 1):
        with pytest.raises(ValueError, match='motion'):
            RE.plan_reenact(photos, frames, box, None, 4, motion=bad)
    for bad in (-0.1, 4.5, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='gain'):
            RE.plan_reenact(photos, frames, box, None, 4, gain=bad)
    with pytest.raises(ValueError, match='feather'):
        RE.plan_reenact(photos, frames, box, None, 4, feather=0.6)
    with pytest.raises(ValueError, match='box_smooth'):
        RE.plan_reenact(photos, frames, box, None, 4, box_smooth=0.0)
    with pytest.raises(ValueError, match='fps'):
        RE.plan_reenact(photos, frames, box, None, 4, fps=0.0)
    with pytest.raises(ValueError, match='chunk_frames'):
        RE.plan_reenact(photos, frames, box, None, 4, chunk_frames=0)
    with pytest.raises(NotImplementedError, match='template'):
        RE.plan_reenact(photos, frames, box, None, 4, template=object())                     # template= passed
    with pytest.raises(NotImplementedError, match='tps'):
        RE.plan_reenact(photos, frames, box, None, 4, model='tps')
    sig = inspect.signature(GEN.ImageGenerator.reenact).parameters
    assert list(sig)[:15] == ['self', 'photos', 'frames', 'driver_box', 'boxes', 'motion', 'rigid', 'gain', 'smooth', 'feather', 'paste',
                              'box_smooth', 'one_euro', 'fps', 'chunk_frames']
    assert [sig[k].default for k in ('boxes', 'motion', 'rigid', 'gain', 'smooth', 'feather', 'paste', 'box_smooth', 'fps', 'chunk_frames')] == [
        None, 'relative', True, 1.0, True, 0.125, True, 0.5, 25.0, 32]
    assert isinstance(sig['one_euro'].default, TR.OneEuro) and sig['return_faces'].default is False and sig['template'].default is None
    r = RE.Reenactment(None, np.array([[0, 1], [1, 0]], dtype=np.int32), None, None, None)
    assert r.held.tolist() == [[False, True], [True, False]]


def test_the_module_imports_without_a_gpu():
    import subprocess
    code = ('import torch; torch.cuda.is_available = lambda: False; import imm_amd.reenact as RE; '
            'print(RE.MOTIONS, RE.FLAG_HELD, callable(RE.plan_reenact), callable(RE.run))')
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-1500:]
    assert "('relative', 'absolute') 1 True True" in out.stdout.decode()


def test_generate_script_lists_the_reenactment_arguments():
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'generate.py'), '--help'], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-1500:]
    text = out.stdout.decode()
    for flag in ('--drive-dir', '--drive-box', '--motion', '--no-rigid', '--gain', '--fps'):
        assert flag in text, flag
