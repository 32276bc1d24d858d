"""Face tracking, host side (no GPU): the ABI of imm_track_step and its argument validation, hand-derived known answers of the numpy
restatement of the rule (tests/track_reference.py), the One-Euro filter's fixed points, and the refusals of plan_track."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_reference as R                                                # noqa: E402

from imm_amd import tracking as TR                                          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 128
BOX = np.array([[0, 100, 200, 228, 328]], dtype=np.int32)                  # 128 x 128: one S x S pixel is one source pixel
HW = np.array([[400, 500]], dtype=np.int32)
ANCHOR = np.array([[132.0, 240.0], [196.0, 264.0], [164.0, 300.0]])         # source pixels; relative to the centre (164, 264):
Z0 = np.array([[-32.0, -24.0], [32.0, 0.0], [0.0, 36.0]])                   # mean (0, 4), sum |z0 - mean|^2 = 3872


def mu_of(points, box=BOX[0], size=S):
    """The landmarks whose source pixels are `points` [K, 2] in `box` (exact in f32 for the integers and boxes used here)."""
    y0, x0, y1, x1 = (float(v) for v in box[1:])
    sc = np.array([(y1 - y0) / size, (x1 - x0) / size])
    mu = ((np.asarray(points, np.float64) - [y0, x0]) / sc) / (size / 2.0) - 1.0
    assert np.array_equal(mu.astype(np.float32).astype(np.float64), mu)
    return mu.astype(np.float32)[None]


def started(beta=1.0, one_euro=None, points=ANCHOR, box=BOX):
    st = R.new_state(1, len(points))
    out = R.track_step(mu_of(points, box[0]), box, HW, st, S, 0, 1, beta, one_euro)
    return st, out


# ----------------------------------------------------------------------------------------------------------------------------
# ABI and validation
# ----------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_track_entry_point():
    from imm_amd import _lib as L
    assert L.ABI_VERSION >= 28
    header = open(os.path.join(ROOT, 'include', 'imm_track.h')).read()
    assert L.symbols('imm_track.h') == ['imm_track_step']
    # the header states the rule the restatement follows: its steps, its clamps and the state layout
    for text in ('THE RULE', 'rounded separately', '4194304', '8388608', 'rint', '[F][5 + 6 K]', 'LOST', 'One-Euro'):
        assert text in header, text
    src = open(os.path.join(ROOT, 'imm_amd', 'csrc', 'track.hip')).read()
    assert 'fp contract(off)' in src and not re.search(r'\b(sin|cos|exp|log|pow|atan2?|tan)f?\s*\(', src), 'no transcendental on the device'


def test_track_step_validates_its_arguments_without_a_device():
    from imm_amd import _lib as L
    lib = L.load()
    one = C.c_void_p(16)                                   # a non-null pointer that is never read: validation comes first
    good = [one, one, one, one, 10, 128, 3, 1, 0, 0, 0.5, 1.0, 0.05, 1.0, 0.25, 0.04, 0, one, one, one, one, one, None]
    nan, inf = float('nan'), float('inf')
    bad_args = [(i, None) for i in (0, 1, 2, 3, 17, 18, 19, 20, 21)]                                    # null pointers
    bad_args += [(6, 0), (6, -1), (6, 65536), (4, 0), (4, 65), (5, 0), (5, 8193)]                        # F, K, S
    bad_args += [(7, 0), (8, -1), (9, 2), (9, -1)]                                                       # n_images, next_image, init
    bad_args += [(10, 0.0), (10, -0.5), (10, 1.5), (10, nan)]                                            # box_smooth outside (0, 1]
    bad_args += [(i, v) for i in (11, 13, 14, 15) for v in (0.0, -1.0, nan, inf)]                        # min_cutoff, d_cutoff, c, te
    bad_args += [(12, -1.0), (12, nan), (12, inf)]                                                       # the One-Euro beta
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert lib.imm_track_step(*args) == -1, (i, bad)
        assert b'track_step' in lib.imm_last_error()


# ----------------------------------------------------------------------------------------------------------------------------
# known answers, K = 3, beta = 1, filter off
# ----------------------------------------------------------------------------------------------------------------------------
def test_anchor_landmarks_leave_the_box_unchanged():
    st, (pts, smooth, rows, geom, flags) = started()
    v = TR.state_views(st[0], 3)
    assert np.array_equal(v['z0'], Z0) and v['h0w0'].tolist() == [128.0, 128.0] and v['box'].tolist() == [164.0, 264.0, 1.0]
    assert np.array_equal(pts[0], ANCHOR) and np.array_equal(smooth, pts) and pts.dtype == np.float32
    assert rows.tolist() == [[0, 100, 200, 228, 328]] and rows.dtype == np.int32 and flags.tolist() == [0]
    assert np.array_equal(geom, [[100.0, 200.0, 1.0, 1.0]]) and geom.dtype == np.float32
    assert R.state_size(3) == TR.state_size(3) == st.shape[1] == 23


def test_a_translation_moves_the_box_by_exactly_that():
    st, _ = started()
    pts, _s, rows, geom, flags = R.track_step(mu_of(ANCHOR + [3.0, -2.0]), BOX, HW, st, S, 7, 0, 1.0)
    assert rows.tolist() == [[7, 103, 198, 231, 326]] and flags.tolist() == [0]                   # and the next image index
    assert TR.state_views(st[0], 3)['box'].tolist() == [167.0, 262.0, 1.0]
    assert np.array_equal(TR.state_views(st[0], 3)['z0'], Z0), 'the anchor is set once'
    assert np.array_equal(pts[0], ANCHOR + [3.0, -2.0]) and np.array_equal(geom, [[103.0, 198.0, 1.0, 1.0]])


def test_a_scaling_doubles_the_sides_about_the_mapped_centre():
    st, _ = started()
    centroid = ANCHOR.mean(axis=0)
    assert centroid.tolist() == [164.0, 268.0]
    _p, _s, rows, geom, flags = R.track_step(mu_of(centroid + 2.0 * (ANCHOR - centroid)), BOX, HW, st, S, 0, 0, 1.0)
    # a = 2, b = centroid - 2 * mean z0 = (164, 268) - (0, 8): the box centre z = 0 maps to (164, 260)
    assert TR.state_views(st[0], 3)['box'].tolist() == [164.0, 260.0, 2.0]
    assert rows.tolist() == [[0, 36, 132, 292, 388]] and flags.tolist() == [0]
    assert np.array_equal(geom, [[36.0, 132.0, 2.0, 2.0]])


def test_a_rotation_by_a_quarter_turn_keeps_the_box():
    st, _ = started()
    rot = np.stack([Z0[:, 1], -Z0[:, 0]], axis=1)                   # z -> i z with z = y + ix: (y, x) -> (-x, y); here -i: also a turn
    for turned in (np.stack([-Z0[:, 1], Z0[:, 0]], axis=1), rot):
        st2 = st.copy()
        _p, _s, rows, _g, flags = R.track_step(mu_of(np.array([164.0, 264.0]) + turned), BOX, HW, st2, S, 0, 0, 1.0)
        assert rows.tolist() == [[0, 100, 200, 228, 328]] and flags.tolist() == [0]
        assert TR.state_views(st2[0], 3)['box'].tolist() == [164.0, 264.0, 1.0]


def test_a_rectangular_box_keeps_its_aspect():
    box = np.array([[0, 10, 20, 74, 148]], dtype=np.int32)              # 64 x 128: sy = 0.5, sx = 1
    pts = np.array([[20.0, 40.0], [60.0, 80.0], [40.0, 120.0]])              # centroid (40, 80)
    st, (p, _s, rows, geom, flags) = started(points=pts, box=box)
    assert np.array_equal(p[0], pts) and rows.tolist() == [[0, 10, 20, 74, 148]] and np.array_equal(geom, [[10.0, 20.0, 0.5, 1.0]])
    c = pts.mean(axis=0)
    _p, _s, rows, geom, _f = R.track_step(mu_of(c + 2.0 * (pts - c), box[0]), box, HW, st, S, 0, 0, 1.0)
    assert (rows[0, 3] - rows[0, 1], rows[0, 4] - rows[0, 2]) == (128, 256) and np.array_equal(geom[0, 2:], [1.0, 2.0])


# ----------------------------------------------------------------------------------------------------------------------------
# the box filter, lost faces, clamps, flags
# ----------------------------------------------------------------------------------------------------------------------------
def test_half_way_with_beta_one_half_and_a_rint_tie():
    st, _ = started(beta=0.5)
    assert TR.state_views(st[0], 3)['box'].tolist() == [164.0, 264.0, 1.0]
    _p, _s, rows, _g, _f = R.track_step(mu_of(ANCHOR + [1.0, -2.0]), BOX, HW, st, S, 0, 0, 0.5)
    assert TR.state_views(st[0], 3)['box'].tolist() == [164.5, 263.0, 1.0]
    # y0' = rint(164.5 - 64) = rint(100.5) = 100: the tie goes to the even integer, not up
    assert rows.tolist() == [[0, 100, 199, 228, 327]]
    _p, _s, rows, _g, _f = R.track_step(mu_of(ANCHOR + [1.0, -2.0]), BOX, HW, st, S, 0, 0, 0.5)
    assert TR.state_views(st[0], 3)['box'].tolist() == [164.75, 262.5, 1.0] and rows.tolist() == [[0, 101, 198, 229, 326]]   # rint(198.5) = 198
    c = ANCHOR.mean(axis=0)
    st, _ = started(beta=0.5)
    _p, _s, rows, _g, _f = R.track_step(mu_of(c + 2.0 * (ANCHOR - c)), BOX, HW, st, S, 0, 0, 0.5)
    assert TR.state_views(st[0], 3)['box'].tolist() == [164.0, 262.0, 1.5] and rows.tolist() == [[0, 68, 166, 260, 358]]


def test_lost_faces_keep_their_state_and_their_box():
    st, _ = started()
    R.track_step(mu_of(ANCHOR + [3.0, -2.0]), BOX, HW, st, S, 0, 0, 1.0)
    before = st.copy()
    prev = np.array([[0, 103, 198, 231, 326]], dtype=np.int32)
    mu = mu_of(ANCHOR + [9.0, 9.0], prev[0])
    for bad in (np.nan, np.inf, -np.inf):
        mu2 = mu.copy()
        mu2[0, 1, 0] = bad
        pts, smooth, rows, geom, flags = R.track_step(mu2, prev, HW, st, S, 5, 0, 1.0)
        assert flags.tolist() == [1] and np.array_equal(st.view(np.int64), before.view(np.int64))
        assert rows.tolist() == [[5, 103, 198, 231, 326]]                      # the previous box with the new image index
        assert not np.isfinite(pts[0, 1, 0]) and np.isfinite(pts[0, 0]).all() and np.isfinite(pts[0, 2]).all()
    # with the filter on, a lost face's points_smooth is the unchanged filter state
    st, _ = started(one_euro=(1.0, 0.05, 1.0))
    before = st.copy()
    mu2 = mu_of(ANCHOR + [9.0, 9.0])
    mu2[0, 2, 1] = np.nan
    _p, smooth, _r, _g, flags = R.track_step(mu2, BOX, HW, st, S, 0, 0, 1.0, (1.0, 0.05, 1.0))
    assert flags.tolist() == [1] and np.array_equal(st.view(np.int64), before.view(np.int64)) and np.array_equal(smooth[0], ANCHOR)
    # an anchor whose points all coincide has no fit: den == 0, lost from the first frame, the box stays
    st, (_p, _s, rows, _g, flags) = started(points=np.tile([[150.0, 250.0]], (3, 1)))
    assert flags.tolist() == [1] and rows.tolist() == BOX.tolist() and TR.state_views(st[0], 3)['box'].tolist() == [164.0, 264.0, 1.0]
    _p, _s, rows, _g, flags = R.track_step(mu_of(ANCHOR), BOX, HW, st, S, 3, 0, 1.0)
    assert flags.tolist() == [1] and rows.tolist() == [[3, 100, 200, 228, 328]]


def test_the_stated_clamps():
    lost = mu_of(ANCHOR)
    lost[0, 0, 0] = np.nan                                       # a lost face: the next box comes from the state as it stands
    for cy, cx, s, want in ((1e12, -1e12, 1e9, [0, 2 ** 23, -2 ** 23, 2 ** 23 + 2 ** 22, -2 ** 23 + 2 ** 22]),
                            (50.0, 60.0, 1e-9, [0, 49, 59, 51, 61]),
                            (np.nan, np.inf, np.nan, [0, -2 ** 23, 2 ** 23, -2 ** 23 + 2, 2 ** 23 + 2]),
                            (0.0, 0.0, -3.0, [0, -1, -1, 1, 1])):
        st, _ = started()
        st[0, 2:5] = [cy, cx, s]
        _p, _s, rows, geom, flags = R.track_step(lost, BOX, HW, st, S, 0, 0, 1.0)
        assert rows.tolist() == [want] and flags[0] & 1
        assert rows[0, 3] > rows[0, 1] and rows[0, 4] > rows[0, 2] and np.abs(rows[0, 1:].astype(np.int64)).max() < 2 ** 24
        assert np.isfinite(geom).all()
    # the same through the measurement: landmarks a billion boxes wide, a trillion pixels away
    st, _ = started()
    big = ((ANCHOR - ANCHOR.mean(axis=0)) * 1e9 + 1e12).astype(np.float32)
    mu = (((big.astype(np.float64) - [100.0, 200.0]) / 64.0) - 1.0).astype(np.float32)[None]
    _p, _s, rows, _g, flags = R.track_step(mu, BOX, HW, st, S, 0, 0, 1.0)
    assert flags.tolist() == [2] and rows.tolist() == [[0, 2 ** 23, 2 ** 23, 2 ** 23 + 2 ** 22, 2 ** 23 + 2 ** 22]]
    v = TR.state_views(st[0], 3)['box']
    assert v[2] > 0.9e9 and v[0] > 0.9e12


def test_the_flag_of_a_box_that_leaves_the_photo():
    hw = np.array([[300, 400], [50, 50]], dtype=np.int32)
    for shift, img, want in (((0.0, 0.0), 0, 0), ((199.0, 0.0), 0, 0), ((200.0, 0.0), 0, 2), ((0.0, 200.0), 0, 2), ((-227.0, 0.0), 0, 0),
                             ((-228.0, 0.0), 0, 2), ((0.0, -328.0), 0, 2), ((0.0, 0.0), 1, 2), ((0.0, 0.0), 2, 2), ((0.0, 0.0), -1, 2)):
        st, _ = started()
        box = BOX.copy()
        box[0, 0] = img
        _p, _s, rows, _g, flags = R.track_step(mu_of(ANCHOR + shift), box, hw, st, S, 0, 0, 1.0)
        assert flags.tolist() == [want], (shift, img, rows)
    tr = TR.Track(None, None, None, None, np.array([[0, 1], [2, 3]], dtype=np.int32))
    assert tr.lost.tolist() == [[False, True], [False, True]] and tr.outside.tolist() == [[False, False], [True, True]]


# ----------------------------------------------------------------------------------------------------------------------------
# the One-Euro filter
# ----------------------------------------------------------------------------------------------------------------------------
def test_one_euro_fixed_points():
    oe = (1.0, 0.05, 1.0)
    st, (pts, smooth, _r, _g, _f) = started(beta=0.5, one_euro=oe)
    assert np.array_equal(smooth, pts), 'the first frame passes through'
    v = TR.state_views(st[0], 3)
    assert np.array_equal(v['xhat'], ANCHOR) and not v['dxhat'].any()
    for _ in range(4):                                                        # a constant input stays constant
        pts, smooth, rows, _g, _f = R.track_step(mu_of(ANCHOR), BOX, HW, st, S, 0, 0, 0.5, oe)
        assert np.array_equal(smooth, pts) and np.array_equal(pts[0], ANCHOR) and rows.tolist() == BOX.tolist()
        assert not TR.state_views(st[0], 3)['dxhat'].any()
    # a step input is followed from behind, monotonically, and the lag closes
    moved = ANCHOR + [4.0, 0.0]
    gap = []
    for _ in range(40):
        pts, smooth, _r, _g, _f = R.track_step(mu_of(moved), BOX, HW, st, S, 0, 0, 1e-9, oe)      # the box (nearly) held still
        gap.append(float(pts[0, 0, 0] - smooth[0, 0, 0]))
        assert np.array_equal(smooth[0, :, 1], ANCHOR[:, 1].astype(np.float32))                    # x never moved
    assert 3.0 < gap[0] < 4.0 and all(a > b > 0 for a, b in zip(gap, gap[1:])) and gap[-1] < 0.01
    # the first step by hand: r = 1 / (1 + 1 / (c fc)), c = 2 pi / 25, speeds in box heights per second
    c = 2 * np.pi / 25.0
    r = lambda fc: 1.0 / (1.0 + 1.0 / (c * fc))
    dxhat = r(1.0) * (4.0 / ((1 / 25.0) * 128.0))
    assert abs(gap[0] - 4.0 * (1.0 - r(1.0 + 0.05 * dxhat))) < 1e-5
    # one_euro=None is the identity whatever the motion
    st, _ = started()
    for shift in ((5.0, 1.0), (-7.0, 2.0), (0.0, 0.0)):
        pts, smooth, _r, _g, _f = R.track_step(mu_of(ANCHOR + shift), BOX, HW, st, S, 0, 0, 1.0, None)
        assert np.array_equal(smooth.view(np.int32), pts.view(np.int32))
    assert np.array_equal(TR.state_views(st[0], 3)['xhat'], ANCHOR), 'the pairs are not touched with the filter off'


def test_one_euro_and_filter_constants_checks():
    oe = TR.OneEuro()
    assert (oe.min_cutoff, oe.beta, oe.d_cutoff) == (1.0, 0.05, 1.0) and 'OneEuro' in repr(oe)
    for kw in ({'min_cutoff': 0.0}, {'min_cutoff': -1.0}, {'d_cutoff': 0.0}, {'d_cutoff': float('nan')}, {'beta': -0.1},
               {'beta': float('inf')}, {'min_cutoff': float('inf')}):
        with pytest.raises(ValueError):
            TR.OneEuro(**kw)
    mc, be, dc, c, te, off = TR.filter_constants(TR.OneEuro(2.0, 0.0, 3.0), 30.0)
    assert (mc, be, dc, off) == (2.0, 0.0, 3.0, 0) and c == 2.0 * np.pi / 30.0 and te == 1.0 / 30.0
    assert TR.filter_constants(None, 25.0)[5] == 1
    with pytest.raises(ValueError, match='one_euro'):
        TR.filter_constants((1.0, 0.05, 1.0), 25.0)


# ----------------------------------------------------------------------------------------------------------------------------
# plan_track
# ----------------------------------------------------------------------------------------------------------------------------
def test_plan_track():
    import inspect
    import torch
    from imm_amd import inference as INF
    frames = [np.zeros((30, 40, 3), np.uint8), np.zeros((20, 25), np.uint8)]
    fr, rows, beta, consts, chunk = TR.plan_track(frames, [(2, 3, 20, 30), (-5, -5, 10, 10)], 4)
    assert rows.tolist() == [[0, 2, 3, 20, 30], [0, -5, -5, 10, 10]] and rows.dtype == np.int32
    assert fr[1].shape == (20, 25, 3) and beta == 0.5 and chunk == 32 and consts[5] == 0
    assert TR.plan_track(frames, [(0, 2, 3, 20, 30)], 1, 1.0, None, 30.0, 2)[2:] == (1.0, TR.filter_constants(None, 30.0), 2)
    with pytest.raises(ValueError, match='max_batch'):
        TR.plan_track(frames, [(2, 3, 20, 30)] * 5, 4)                                     # F > max_batch
    with pytest.raises(ValueError, match='frame 0'):
        TR.plan_track(frames, [(0, 2, 3, 20, 30), (1, 2, 3, 20, 30)], 4)                    # a row naming frame 1
    with pytest.raises(ValueError, match='no frames'):
        TR.plan_track([], [(2, 3, 20, 30)], 4)
    with pytest.raises(ValueError, match='no boxes'):
        TR.plan_track(frames, [], 4)
    with pytest.raises(ValueError, match='empty'):
        TR.plan_track(frames, [(2, 3, 2, 30)], 4)
    for tensor in (torch.zeros(2, 128, 128, 3), np.zeros((2, 30, 40, 3), np.uint8)):
        with pytest.raises(ValueError, match='list of u8'):
            TR.plan_track(tensor, [(2, 3, 20, 30)], 4)
    with pytest.raises(ValueError, match='uint8'):
        TR.plan_track([np.zeros((30, 40, 3), np.float32)], [(2, 3, 20, 30)], 4)
    for bad in (0.0, -0.5, 1.01, float('nan')):
        with pytest.raises(ValueError, match='box_smooth'):
            TR.plan_track(frames, [(2, 3, 20, 30)], 4, box_smooth=bad)
    for bad in (0.0, -25.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='fps'):
            TR.plan_track(frames, [(2, 3, 20, 30)], 4, fps=bad)
    with pytest.raises(ValueError, match='chunk_frames'):
        TR.plan_track(frames, [(2, 3, 20, 30)], 4, chunk_frames=0)
    sig = inspect.signature(INF.LandmarkDetector.track).parameters
    assert list(sig) == ['self', 'frames', 'boxes', 'regressor', 'box_smooth', 'one_euro', 'fps', 'chunk_frames']
    assert (sig['regressor'].default, sig['box_smooth'].default, sig['fps'].default, sig['chunk_frames'].default) == (None, 0.5, 25.0, 32)
    assert isinstance(sig['one_euro'].default, TR.OneEuro) and hasattr(INF.LandmarkDetector, 'tracker')
    for name in ('start', 'step', 'result'):
        assert callable(getattr(TR.FaceTracker, name))


def test_detect_script_lists_the_tracking_arguments():
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'detect.py'), '--help'], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-1500:]
    text = out.stdout.decode()
    for flag in ('--track', '--fps', '--box-smooth', '--no-filter'):
        assert flag in text, flag
