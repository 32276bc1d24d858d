"""Clip morph, host side (no GPU): the ABI of imm_clip_rows / imm_clip_ema and their argument validation, the wrapper and plan_clip
refusals, the numpy restatement of the two rules (tests/clip_reference.py) against the host functions it replaces and the tracker's
step it inverts, the filter's properties, and the script's arguments."""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_reference as CR                                                 # noqa: E402
import track_reference as TRR                                               # noqa: E402

from imm_amd import clip as CL                                              # noqa: E402  (imports without a GPU)
from imm_amd import generation as GN                                        # noqa: E402
from imm_amd import morphing as MP                                          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
NAMES = ['imm_clip_ema', 'imm_clip_rows']


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


# ----------------------------------------------------------------------------------------------------------------------------
# ABI and validation
# ----------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_clip_entry_points():
    from imm_amd import _lib as L
    assert L.ABI_VERSION >= 35
    header = open(os.path.join(ROOT, 'include', 'imm_clip.h')).read()
    assert L.symbols('imm_clip.h') == NAMES
    for text in ('THE RULE', 'Rows (imm_clip_rows)', 'Filter (imm_clip_ema)', 'rounded separately', 'r <= 0.5 ? 2 : 1 / fmax(r, 0.5)',
                 'generation.compose_inv_ramp', 'morphing.hull_inv_soft', 'LOST', 'every value is NaN', 'the inverse of step 1 of imm_track.h',
                 '(double)((float)H / (float)S)', 'fmin(fmax(v, -1), 1)', 'SKIPPED', 'seen[i] = 1', 'Consequences', '(a)', '(b)', '(c)', '(d)',
                 'a fixed point in its bits', '1 <= F <= 65535, 1 <= K <= 80', 'validated before any HIP call'):
        assert text in header, text
    src = open(os.path.join(ROOT, 'imm_amd', 'csrc', 'clip.hip')).read()
    assert 'fp contract(off)' in src and 'atomic' not in src.lower() and 'asm' not in src.lower()
    for fn in ('clip_inv_ramp', 'clip_inv_soft', 'clip_scale', 'clip_landmark', 'clip_rows_kernel', 'clip_ema_one'):
        body = src[re.search(r'\b%s\(' % fn, src).start():]
        assert 'fp contract(off)' in body[:body.index('\n}\n')], fn
    for fn in ('cos', 'sin', 'tan', 'exp', 'log', 'pow', 'sqrt'):
        assert not re.search(r'\b%sf?\s*\(' % fn, src), 'only + - * / fmin fmax run on the device: %s' % fn
    assert "'*.hip'" in open(os.path.join(ROOT, 'imm_amd', 'build.py')).read(), 'build.py globs the sources'
    assert 'the two clip calls of `include/imm_clip.h`' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_clip_entry_points_validate_their_arguments_without_a_device():
    from imm_amd import _lib as L
    lib = L.load()
    one, two, far = C.c_void_p(16), C.c_void_p(32), C.c_void_p(1 << 30)   # non-null pointers that are never read: validation comes first
    #       boxes flags mu  points K  S    F  feather mask_feather own inv_ramp inv_soft stream
    good = [one, one, one, one, 10, 128, 3, 0.125, one, two, two, two, None]
    bad_args = [(i, None) for i in (0, 1, 2, 8, 9, 10, 11)]               # mask_feather without inv_soft and the reverse are refused too
    bad_args += [(4, 0), (4, 81), (4, -1), (5, 0), (5, 8193), (6, 0), (6, -3), (6, 65536), (7, -0.01), (7, 0.51), (7, float('nan')),
                 (7, float('inf'))]
    for points in (one, None):                                            # points is nullable
        for i, bad in bad_args:
            args = list(good)
            args[3] = points
            args[i] = bad
            assert lib.imm_clip_rows(*args) == -1, (i, bad)
            assert b'clip_rows' in lib.imm_last_error()
    #       x    state seen skip lost n  width alpha stream
    good = [one, far, one, one, one, 3, 6, 0.25, None]
    bad_args = [(i, None) for i in (0, 1, 2, 3)]
    bad_args += [(5, 0), (5, -1), (5, 65536), (6, 0), (6, 769), (6, -6), (7, 0.0), (7, -0.25), (7, 1.5), (7, float('nan')), (7, float('inf')),
                 (1, one), (1, C.c_void_p(16 + 4 * 17)), (0, C.c_void_p((1 << 30) + 4))]     # x and state overlap
    for lost in (one, None):                                              # lost is nullable
        for i, bad in bad_args:
            args = list(good)
            args[4] = lost
            args[i] = bad
            assert lib.imm_clip_ema(*args) == -1, (i, bad)
            assert b'clip_ema' in lib.imm_last_error()


def test_wrapper_refusals_come_before_any_device_call():
    from imm_amd import ops
    z = lambda *sh, **kw: torch.zeros(*sh, **kw)           # host tensors: a wrapper that got as far as the library would fault
    F, K = 3, 10
    i32 = dict(dtype=torch.int32)
    rows = dict(boxes=z(F, 5, **i32), track_flags=z(F, **i32), mu=z(F, K, 2), points=z(F, K, 2), image_size=128, feather=0.125,
                mask_feather=z(F), own=z(F, K, 2), inv_ramp=z(F, 2), inv_soft=z(F))
    shared = z(F, K, 2)
    for kw, match in ((dict(mu=z(F, K)), 'mu'), (dict(mu=z(F, 81, 2), own=z(F, 81, 2), points=None), 'clip_rows serves'),
                      (dict(boxes=z(F, 4, **i32)), 'boxes'), (dict(boxes=z(F, 5)), 'boxes'), (dict(track_flags=z(F + 1, **i32)), 'track_flags'),
                      (dict(points=z(F, K, 3)), 'points'), (dict(points=z(F, K, 2).double()), 'points'), (dict(own=z(F, K + 1, 2)), 'own'),
                      (dict(inv_ramp=z(F)), 'inv_ramp'), (dict(inv_soft=z(F, 1)), 'inv_soft'), (dict(mask_feather=z(F).double()), 'mask_feather'),
                      (dict(mask_feather=None), 'exactly when'), (dict(inv_soft=None), 'exactly when'), (dict(feather=0.6), 'feather'),
                      (dict(feather=float('nan')), 'feather'), (dict(image_size=0), 'image_size'), (dict(mu=shared, own=shared), 'overlaps'),
                      (dict(points=shared, own=shared), 'overlaps')):
        with pytest.raises(ValueError, match=match):
            ops.clip_rows(**dict(rows, **kw))
    n, width = 3, 6
    ema = dict(x=z(n, width), state=z(n, width), seen=z(n, **i32), skip=z(n, **i32), lost=z(n, **i32), alpha=0.25)
    both = z(n, width)
    for kw, match in ((dict(x=z(n)), 'x must be'), (dict(x=z(n, 769), state=z(n, 769)), 'clip_ema serves'), (dict(state=z(n, width + 1)), 'state'),
                      (dict(state=z(n, width).double()), 'state'), (dict(seen=z(n)), 'seen'), (dict(skip=z(n + 1, **i32)), 'skip'),
                      (dict(lost=z(n, 1, **i32)), 'lost'), (dict(x=both, state=both), 'overlaps'), (dict(alpha=0.0), 'alpha'),
                      (dict(alpha=1.01), 'alpha'), (dict(alpha=float('nan')), 'alpha')):
        with pytest.raises(ValueError, match=match):
            ops.clip_ema(**dict(ema, **kw))


# ----------------------------------------------------------------------------------------------------------------------------
# plan_clip and the script's arguments
# ----------------------------------------------------------------------------------------------------------------------------
def test_plan_clip_checks_its_arguments():
    frames = [np.zeros((40, 50, 3), np.uint8), np.zeros((30, 36, 3), np.uint8)]
    donors = [np.zeros((20, 25, 3), np.uint8), np.zeros((35, 30), np.uint8)]
    faces = [(2, 3, 30, 40), (5, 5, 25, 20)]
    good = dict(frames=frames, boxes=faces, donors=donors, K=10, max_batch=4)
    plan = CL.plan_clip(**good)
    assert len(plan.frames) == 2 and plan.rows.tolist() == [[0, 2, 3, 30, 40], [0, 5, 5, 25, 20]] and plan.rows.dtype == np.int32
    assert plan.morph.shape.tolist() == [0.0, 0.0] and plan.morph.texture.tolist() == [1.0, 1.0], 'the defaults are the swap'
    assert (plan.smooth, plan.colour_smooth, plan.seam_smooth, plan.box_smooth, plan.chunk_frames) == (True, 0.25, 0.25, 0.5, 32)
    assert isinstance(plan.morph, MP.MorphPlan) and plan.morph.donor_rows.shape == (2, 5) and plan.morph.rows.tolist() == plan.rows.tolist()
    one = CL.plan_clip(**dict(good, donors=donors[:1], colour_smooth=1, seam_smooth=1.0, smooth=False, mask='hull', seamless=[0.0, 1.0]))
    assert one.morph.donor_rows.tolist() == [[0, 0, 0, 20, 25]] * 2 and one.colour_smooth == 1.0 and one.smooth is False
    for kw, match in ((dict(frames=[]), 'no frames'), (dict(frames=np.zeros((2, 40, 50, 3), np.uint8)), 'list of u8'),
                      (dict(donors=donors + donors[:1]), '3 donors for 2 faces'), (dict(donors=[]), 'donors'),
                      (dict(boxes=faces + faces + faces[:1]), 'max_batch'), (dict(boxes=[(1, 2, 3, 30, 40)]), 'image index 0'),
                      (dict(seamless=0.5), "needs mask='hull'"), (dict(mask='box'), 'mask'), (dict(shape=1.5), 'shape'),
                      (dict(texture=[0.5] * 3), 'texture'), (dict(feather=0.6), 'feather'), (dict(colour=-1), 'colour'), (dict(max_gain=0.5), 'max_gain'),
                      (dict(grow=0), 'grow'), (dict(ring=8), 'ring'), (dict(anchors=40), 'anchors|control points'), (dict(box_smooth=0), 'box_smooth'),
                      (dict(fps=0), 'fps'), (dict(chunk_frames=0), 'chunk_frames'), (dict(one_euro=3), 'one_euro'),
                      (dict(donor_landmarks=torch.zeros(2, 9, 2)), 'donor_landmarks')):
        with pytest.raises(ValueError, match=match):
            CL.plan_clip(**dict(good, **kw))
    for name in ('colour_smooth', 'seam_smooth'):
        for bad in (0, 0.0, -0.25, 1.01, float('nan'), float('inf'), None, 'fast'):
            with pytest.raises(ValueError, match=name):
                CL.plan_clip(**dict(good, **{name: bad}))
    assert CL.grid_pixels(plan.rows) == 4 * 28 * 37 and CL.grid_pixels(np.array([[0, 0, 0, 1 << 20, 1 << 20]])) == 2 ** 31 - 1
    cm = CL.ClipMorph([1, 2], None, np.zeros((2, 3, 10, 2)), None)
    assert len(cm) == 2 and cm.colour_gain is None and cm.seam_diff is None and cm.hull_flags is None
    doc = CL.__doc__ + CL.ClipMorph.__doc__
    assert 'nobody has tuned them' in doc and 'imports without a GPU' in doc


def test_generate_script_parses_the_clip_arguments(capsys):
    spec = importlib.util.spec_from_file_location('generate_script', os.path.join(ROOT, 'scripts', 'generate.py'))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    need = ['--configs', 'c.yaml', '--checkpoint', 'm.pt', '--appearance-dir', 'clip']
    args = script.build_parser().parse_args(need + ['--morph'])
    assert (args.clip, args.no_smooth, args.colour_smooth, args.seam_smooth, args.fps) == (False, False, None, None, 25.0)
    args = script.build_parser().parse_args(need + ['--morph', '--clip', '--no-smooth', '--colour-smooth', '0.5', '--seam-smooth', '1', '--fps', '30'])
    assert (args.clip, args.no_smooth, args.colour_smooth, args.seam_smooth, args.fps) == (True, True, 0.5, 1.0, 30.0)
    for bad in (['--colour-smooth'], ['--seam-smooth', 'slow'], ['--clip', 'yes']):
        with pytest.raises(SystemExit):
            script.build_parser().parse_args(need + ['--morph'] + bad)
    capsys.readouterr()
    for text in ('--morph --clip', '--no-smooth', '--colour-smooth A', '--seam-smooth A', 'untuned'):
        assert text in script.__doc__, text


# ----------------------------------------------------------------------------------------------------------------------------
# the rows
# ----------------------------------------------------------------------------------------------------------------------------
EDGE_ROWS = [(0, 0, 0, 2, 2), (0, 5, 7, 7, 68), (0, -40, -13, 21, -11), (0, 0, 0, 4194304, 4194304), (0, -2097152, 3, 2097152, 64),
             (0, -8388608, 8388607, -8388606, 8388608 + 60), (0, 10, 10, 11, 13), (0, 3, 4, 8, 9)]


def test_restated_ramp_and_softness_are_the_host_functions_bit_for_bit():
    """inv_ramp against generation.compose_inv_ramp and inv_soft against morphing.hull_inv_soft, in their bits: random rows, the edge
    rows (sides 1, 2, 5, 61 and 4194304, negative and extreme coordinates), every feather and mask_feather that bounds a branch."""
    rng = np.random.RandomState(0)
    n = 400
    y0, x0 = rng.randint(-500, 2000, n), rng.randint(-500, 2000, n)
    rand = np.stack([np.zeros(n, int), y0, x0, y0 + rng.randint(1, 900, n), x0 + rng.randint(1, 900, n)], axis=1)
    rows = np.concatenate([rand, np.array(EDGE_ROWS)]).astype(np.int32)
    F = len(rows)
    mu, flags = np.zeros((F, 1, 2), F32), np.zeros(F, np.int32)
    for feather in (0.0, 0.125, 0.25, 0.3, 0.5, 1e-9, 0.1 + 0.2):
        for mf in (0.0, 0.1, 0.5, 1.0, 1e-8):
            feathers = np.full(F, mf, F32) if mf != 0.5 else rng.uniform(0, 1, F).astype(F32)
            _own, ramp, soft = CR.clip_rows(rows, flags, mu, None, 128, feather, feathers)
            assert ramp.dtype == F32 and soft.dtype == F32
            assert np.array_equal(bits(ramp), bits(GN.compose_inv_ramp(rows, feather))), feather
            assert np.array_equal(bits(soft), bits(MP.hull_inv_soft(rows, feathers))), mf
    _own, ramp, soft = CR.clip_rows(rows, flags, mu, None, 128, 0.125, None)
    assert soft is None
    assert ramp[n].tolist() == [2.0, 2.0] and ramp[n + 1].tolist() == [2.0, F32(1.0 / (0.125 * 61))], 'a ramp of <= 0.5 pixels is a hard paste'
    # an empty box (the tracker never makes one; a caller of the kernel may): the rule still has an answer
    empty = np.array([(0, 5, 5, 5, 9), (0, 9, 9, 4, 4)], np.int32)
    _own, ramp, soft = CR.clip_rows(empty, flags[:2], mu[:2], None, 128, 0.25, np.full(2, 0.5, F32))
    assert ramp.tolist() == [[2.0, 1.0], [2.0, 2.0]] and soft.tolist() == [1.0, 1.0]


@pytest.mark.parametrize('side', [2, 61, 4194304])
def test_restated_own_inverts_the_trackers_step_1(side):
    """own = the inverse of step 1 of imm_track.h: the tracker's points (track_reference.track_step, filter off: the stored f32 source
    pixels) of a box of this side, brought back by the restatement, are mu within 2 f32 ulps.
    The bound, derived: the only loss is the rounding of the source pixel p to f32, at most 2^-24 |p| pixels, which is
    2^-24 (2 |y0| / H + mu + 1) in the frame of the box, and the rounding of the result to f32, at most 2^-25 for |mu| < 1; the f64
    operations add 2^-50.  With the box origin within half a side of zero, as here, that is 3.5 * 2^-24 < 2 * 2^-23: two ulps of the
    frame [-1, 1].  (An ulp of mu's own magnitude cannot hold near mu = 0, where p keeps 24 bits of (mu + 1) and not of mu.)"""
    rng = np.random.RandomState(side % 1000)
    F, K, S = 6, 10, 128
    origin = np.array([(0, 0), (-(side // 2), side // 2), (side // 2, -(side // 2)), (-1, 1), (0, -(side // 3)), (side // 4, 0)])
    rows = np.concatenate([np.zeros((F, 1), int), origin, origin + side], axis=1).astype(np.int32)
    mu = rng.uniform(-1, 1, (F, K, 2)).astype(F32)
    mu[0, :4] = [(-1.0, 1.0), (0.0, -0.0), (0.999999, -0.999999), (1e-6, -1e-6)]
    st = TRR.new_state(F, K)
    pts, smooth, _rows, _geom, flags = TRR.track_step(mu, rows, [(side, side)], st, S, 0, 1, 0.5, None, 25.0)
    assert not (flags & 1).any() and np.array_equal(bits(pts), bits(smooth))
    own, _ramp, _soft = CR.clip_rows(rows, flags, mu, pts, S, 0.125, None)
    assert own.dtype == F32 and np.isfinite(own).all() and np.abs(own).max() <= 1.0
    err = np.abs(own.astype(F64) - mu.astype(F64)).max()
    print('\nCLIP own vs mu, side %d: max |error| %.3g = %.2f f32 ulps of the frame' % (side, err, err / 2.0 ** -23))
    assert err <= 2.0 * 2.0 ** -23
    # without points: mu's bits; a lost face: NaN whatever it holds; a point outside the box: the clamp; non-finite points pass
    same, _r, _s = CR.clip_rows(rows, flags, mu, None, S, 0.125, None)
    assert np.array_equal(bits(same), bits(mu))
    lost = flags.copy()
    lost[1] = 3
    for points in (pts, None):
        dropped, _r, _s = CR.clip_rows(rows, lost, mu, points, S, 0.125, None)
        assert np.isnan(dropped[1]).all() and np.isfinite(dropped[[0, 2, 3, 4, 5]]).all()
    far = pts.copy()
    far[2, 0] = [rows[2, 1] - 5.0 * side, rows[2, 4] + 0.75 * side]
    far[2, 1] = [np.nan, np.inf]
    far[2, 2] = [-np.inf, rows[2, 2] + side / 2.0]
    got, _r, _s = CR.clip_rows(rows, flags, mu, far, S, 0.125, None)
    assert got[2, 0].tolist() == [-1.0, 1.0] and np.isnan(got[2, 1, 0]) and got[2, 1, 1] == np.inf and got[2, 2, 0] == -np.inf
    assert abs(float(got[2, 2, 1])) <= 2.0 ** -22


# ----------------------------------------------------------------------------------------------------------------------------
# the filter
# ----------------------------------------------------------------------------------------------------------------------------
def test_filter_properties():
    rng = np.random.RandomState(5)
    n, width = 4, 6
    raw = rng.uniform(-3, 3, (5, n, width)).astype(F32)
    none = np.zeros((5, n), np.int32)
    # (a) the first value passes in its bits, whatever alpha; alpha = 1 keeps following the input within rounding
    for alpha in (0.25, 1.0):
        out = CR.ema_frames(raw, none, none, alpha)
        assert out.dtype == F32 and np.array_equal(bits(out[0]), bits(raw[0]))
    assert np.abs(CR.ema_frames(raw, none, none, 1.0) - raw).max() <= 2 ** -21
    # the recurrence by hand, in f32
    out = CR.ema_frames(raw, none, none, 0.25)
    s = raw[0].copy()
    for t in range(1, 5):
        s = s + F32(0.25) * (raw[t] - s)
        assert s.dtype == F32 and np.array_equal(bits(out[t]), bits(s))
    # (b) a constant input is a fixed point bit for bit, at awkward values and alphas
    const = np.tile(np.array([0.1, -1e-30, 3e38, 1.0 + 2 ** -23, 0.0, 255.0], F32), (5, n, 1))
    for alpha in (0.25, 1.0 / 3.0, 0.9999999, 1.0):
        assert np.array_equal(bits(CR.ema_frames(const, none, none, alpha)), bits(const)), alpha
    zero = CR.ema_frames(np.full((3, 1, 1), -0.0, F32), none[:3, :1], none[:3, :1], 0.25)
    assert np.signbit(zero[0]).all() and not np.signbit(zero[1:]).any() and not zero.any(), 'the one exception: -0 + 0 is +0, the same value'
    # (c) a skipped row changes nothing: x, state and seen stay; the next frame is filtered against the last unskipped one
    x, state, seen = raw[1].copy(), raw[0].copy(), np.array([1, 1, 0, 1], np.int32)
    before = (x.copy(), state.copy(), seen.copy())
    CR.clip_ema(x, state, seen, np.array([0, 4, 1, 0], np.int32), np.array([0, 0, 0, 1], np.int32), 0.25)
    for i in (1, 2, 3):
        assert np.array_equal(bits(x[i]), bits(before[0][i])) and np.array_equal(bits(state[i]), bits(before[1][i])) and seen[i] == before[2][i]
    assert np.array_equal(bits(x[0]), bits(state[0])) and not np.array_equal(x[0], before[0][0]) and seen.tolist() == [1, 1, 0, 1]
    x2, st2, seen2 = raw[1].copy(), raw[0].copy(), np.ones(n, np.int32)
    CR.clip_ema(x2, st2, seen2, np.zeros(n, np.int32), np.array([2, 2, 2, 2], np.int32), 0.25)
    assert np.array_equal(bits(x2[0]), bits(x[0])), 'bit 1 of lost (the box left the photo) does not skip; lost=None reads nothing'
    x3, st3, seen3 = raw[1].copy(), raw[0].copy(), np.ones(n, np.int32)
    CR.clip_ema(x3, st3, seen3, np.zeros(n, np.int32), None, 0.25)
    assert np.array_equal(bits(x3), bits(x2))
    skips = np.zeros((5, n), np.int32)
    skips[0, 1] = 1                                                           # skipped on the first frame: frame 1 is its first value
    skips[2, 0] = 1                                                           # skipped mid-clip
    out = CR.ema_frames(raw, skips, none, 0.25)
    assert np.array_equal(bits(out[0, 1]), bits(raw[0, 1])) and np.array_equal(bits(out[1, 1]), bits(raw[1, 1]))
    assert np.array_equal(bits(out[2, 0]), bits(raw[2, 0])), 'a skipped row keeps its raw value'
    want = out[1, 0] + F32(0.25) * (raw[3, 0] - out[1, 0])
    assert np.array_equal(bits(out[3, 0]), bits(want)), 'the state did not age over the skipped frame'
    # (d) a NaN stays
    nan = raw.copy()
    nan[1, 3, 2] = np.nan
    out = CR.ema_frames(nan, none, none, 0.25)
    assert np.isnan(out[1:, 3, 2]).all() and np.isfinite(np.delete(out.reshape(5, -1), 3 * width + 2, axis=1)).all()
