"""The seamless morph, host side (no GPU): the ABI of imm_seam_fit / imm_morph_seam_u8 and their argument validation, the wrapper and
plan_morph refusals, the properties of the ring and of the mean-value coordinates of the restatement (tests/seam_reference.py), the
flat-photo known answer, and the f32 restatement of the morph with the membrane against the f64 one on the GPU test's cases."""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_reference as HR                                                 # noqa: E402
import morph_reference as R                                                 # noqa: E402
import seam_reference as SR                                                 # noqa: E402
import unalign_reference as UR                                              # noqa: E402
import warp_reference as WR                                                 # noqa: E402

from imm_amd import morphing as MP                                          # noqa: E402  (imports without a GPU)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
NAMES = ['imm_morph_seam_u8', 'imm_seam_fit']


# ----------------------------------------------------------------------------------------------------------------------------
# ABI and validation
# ----------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_seam_entry_points():
    from imm_amd import _lib as L
    assert L.ABI_VERSION >= 34
    header = open(os.path.join(ROOT, 'include', 'imm_seam.h')).read()
    assert L.symbols('imm_seam.h') == NAMES
    for text in ('THE RULE', 'Seam fit (imm_seam_fit)', 'Ring.', 'Difference.', 'Morph with the membrane (imm_morph_seam_u8)',
                 'rounded separately', 'ORIENTATION', '(1, 0, 0), (-1, 0, H - 1), (0, 1, 0), (0, -1, W - 1)', 'bit 0', 'bit 1',
                 'the lowest such s', 'not clamped', 'correctly rounded', 'never reach an address', 'Consequences', '(a)', '(b)', '(c)', '(d)',
                 'What the rule does NOT do'):
        assert text in header, text
    src = open(os.path.join(ROOT, 'imm_amd', 'csrc', 'seam.hip')).read()
    assert 'fp contract(off)' in src and 'atomic' not in src.lower() and 'asm' not in src.lower()
    for fn in ('cos', 'sin', 'tan', 'atan2', 'acos'):
        assert not re.search(r'\b%sf?\s*\(' % fn, src), 'no transcendental function runs on the device: %s' % fn
    morph = open(os.path.join(ROOT, 'imm_amd', 'csrc', 'morph.hip')).read()
    assert 'imm_morph_seam_u8' in morph and 'bool SEAM = false' in morph and 'bool HULL = false' in morph
    assert 'morph_u8_kernel<true>' in morph and 'morph_u8_kernel<false>' in morph, 'the two earliest launches keep their spelling'
    # every f32 helper the rule runs through carries the pragma itself
    for path, helpers in (('morph.hip', ('seam_field', 'hull_weight')), ('morph_common.h', ('morph_mix', 'morph_donor_place')),
                          ('paste_common.h', ('spline_sum', 'spline_displace', 'spline_displace_at', 'paste_sample_photo', 'paste_blend')),
                          ('seam.hip', ('seam_line', 'seam_ring', 'seam_diff'))):
        text = open(os.path.join(ROOT, 'imm_amd', 'csrc', path)).read()
        for fn in helpers:
            body = text[re.search(r'\b%s\(' % fn, text).start():]
            assert 'fp contract(off)' in body[:body.index('\n}\n')], (path, fn)
    # sqrtf and / stay the correctly rounded ones: the build passes no switch that relaxes them
    build = open(os.path.join(ROOT, 'imm_amd', 'build.py')).read()
    for switch in ('fast-math', 'fhip-fp32-correctly-rounded', 'ffp-contract', 'funsafe-math', 'freciprocal', 'Ofast', 'fapprox'):
        assert switch not in build, switch


def test_seam_entry_points_validate_their_arguments_without_a_device():
    from imm_amd import _lib as L
    lib = L.load()
    one, two, three = C.c_void_p(16), C.c_void_p(32), C.c_void_p(48)     # non-null pointers that are never read: validation comes first
    #       poses boxes grow edges hflags dirs src offs hw n_img donor doffs dhw n_donor dboxes texture ctrl coef_a coef_b gain K  M   B   n
    good = [one, one, one, one, one, one, one, one, one, 2, one, one, one, 3, one, one, one, one, one, one, 10, 18, 128, 3,
            two, two, three, None]                                       # ring diff flags stream
    bad_args = [(i, None) for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 14, 15, 16, 17, 18, 24, 25, 26)]
    bad_args += [(9, 0), (13, 0), (13, -1), (20, 0), (20, 81), (21, 2), (21, 81), (22, 15), (22, 257), (22, 0), (22, -128), (23, 0),
                 (23, -1), (23, 65536)]
    for gain in (one, None):                                             # gain is nullable
        for i, bad in bad_args:
            args = list(good)
            args[19] = gain
            args[i] = bad
            assert lib.imm_seam_fit(*args) == -1, (i, bad)
            assert b'seam_fit' in lib.imm_last_error()
    #       src  dst  offs hw  n_img donor doffs dhw n_donor boxes dboxes links ramp texture ctrl coef_a coef_b gain edges soft ring diff seamless
    good = [one, two, one, one, 2, three, one, one, 3, one, one, one, one, one, one, one, one, one, one, one, one, one, one,
            10, 18, 128, 3, 100, None]                                   # K M B n pixels stream
    bad_args = [(i, None) for i in (0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 18, 19, 20, 21, 22)]
    bad_args += [(1, one), (5, two), (4, 0), (8, 0), (8, -1), (23, 0), (23, 81), (24, 2), (24, 81), (25, 15), (25, 257), (25, 0), (26, 0),
                 (26, 65536), (27, 0), (27, -5)]
    for gain in (one, None):
        for i, bad in bad_args:
            args = list(good)
            args[17] = gain
            args[i] = bad
            assert lib.imm_morph_seam_u8(*args) == -1, (i, bad)
            assert b'morph_seam_u8' in lib.imm_last_error()


def test_wrapper_refusals_come_before_any_device_call():
    from imm_amd import ops
    z = lambda *sh, **kw: torch.zeros(*sh, **kw)           # host tensors: a wrapper that got as far as the library would fault
    n, K, M, B = 2, 10, 18, 16
    i32 = dict(dtype=torch.int32)
    src, dst, don = z(64, dtype=torch.uint8), z(64, dtype=torch.uint8), z(48, dtype=torch.uint8)
    offs, hw, doffs, dhw = z(1, dtype=torch.int64), z(1, 2, **i32), z(2, dtype=torch.int64), z(2, 2, **i32)
    fit = dict(poses=z(n, K, 2), boxes=z(n, 5, **i32), grow=z(n), edges=z(n, K, 3), hull_flags=z(n, **i32), dirs=z(B, 2, dtype=torch.float64),
               src=src, offsets=offs, hw=hw, donor=don, donor_offsets=doffs, donor_hw=dhw, donor_boxes=z(n, 5, **i32), texture=z(n),
               ctrl=z(n, M, 2), coef_a=z(n, M + 3, 2), coef_b=z(n, M + 3, 2), gain=None, ring=z(n, B, 2), diff=z(n, B, 3), flags=z(n, **i32))
    for kw, match in ((dict(poses=z(n, K)), 'poses'), (dict(poses=z(n, 81, 2)), 'landmarks'), (dict(ring=z(n, 15, 2)), 'ring'),
                      (dict(ring=z(n, 257, 2)), 'ring'), (dict(ring=z(n, B, 3)), 'ring'), (dict(ring=z(n, B)), 'ring'),
                      (dict(diff=z(n, B, 2)), 'diff'), (dict(diff=z(n, B + 1, 3)), 'diff'), (dict(dirs=z(B, 2)), 'dirs'),
                      (dict(dirs=z(B + 1, 2, dtype=torch.float64)), 'dirs'), (dict(edges=z(n, K, 2)), 'edges'),
                      (dict(hull_flags=z(n)), 'hull_flags'), (dict(flags=z(n + 1, **i32)), 'flags'), (dict(gain=z(n, 3)), 'gain'),
                      (dict(ctrl=z(n, 2, 2)), 'seam_fit serves'), (dict(coef_a=z(n, M, 2)), 'coef_a'), (dict(texture=z(n, 1)), 'texture'),
                      (dict(grow=z(n).double()), 'grow')):
        with pytest.raises(ValueError, match=match):
            ops.seam_fit(**dict(fit, **kw))
    paste = dict(src=src, dst=dst, offsets=offs, hw=hw, donor=don, donor_offsets=doffs, donor_hw=dhw, boxes=z(n, 5, **i32),
                 donor_boxes=z(n, 5, **i32), links=z(n, 2, **i32), inv_ramp=z(n, 2), texture=z(n), ctrl=z(n, M, 2), coef_a=z(n, M + 3, 2),
                 coef_b=z(n, M + 3, 2), gain=None, edges=z(n, K, 3), inv_soft=z(n), ring=z(n, B, 2), diff=z(n, B, 3), seamless=z(n),
                 max_box_pixels=9)
    for kw, match in ((dict(ring=z(n, 15, 2)), 'ring'), (dict(ring=z(n, B, 2).double()), 'ring'), (dict(diff=z(n, B, 2)), 'diff'),
                      (dict(seamless=z(n, 1)), 'seamless'), (dict(seamless=z(n).double()), 'seamless'), (dict(edges=z(n, 81, 3)), 'edges'),
                      (dict(inv_soft=z(n + 1)), 'inv_soft'), (dict(gain=z(n, 3)), 'gain'), (dict(dst=src), 'copy of src'),
                      (dict(donor=dst), 'never dst'), (dict(max_box_pixels=0), 'max_box_pixels')):
        with pytest.raises(ValueError, match=match):
            ops.morph_seam_u8(**dict(paste, **kw))


# ----------------------------------------------------------------------------------------------------------------------------
# plan_morph, PhotoMorph and the script's arguments
# ----------------------------------------------------------------------------------------------------------------------------
def test_plan_morph_checks_seamless_and_ring():
    photos = [np.zeros((40, 50, 3), np.uint8), np.zeros((30, 30, 3), np.uint8)]
    donors = [np.zeros((20, 25, 3), np.uint8), np.zeros((35, 30), np.uint8)]
    good = dict(photos=photos, donors=donors, boxes=None, donor_boxes=None, shape=0.5, texture=None, feather=0.125, K=10)
    plan = MP.plan_morph(**good)
    assert len(vars(plan)) == 21 and plan.seamless.tolist() == [0.0, 0.0] and plan.seamless.dtype == F32 and plan.ring == 128
    plan = MP.plan_morph(mask='hull', seamless=[0.0, 1.0], ring=16, **good)
    assert len(vars(plan)) == 21 and plan.seamless.tolist() == [0.0, 1.0] and plan.ring == 16 and plan.mask == 'hull'
    assert MP.plan_morph(seamless=0.0, ring=256, **good).ring == 256, 'seamless = 0 needs no mask'
    for kw, match in ((dict(seamless=0.5), "needs mask='hull'"), (dict(seamless=[0.0, 0.01]), "needs mask='hull'"),
                      (dict(mask=None, seamless=1.0), "needs mask='hull'")):
        with pytest.raises(ValueError, match=match):
            MP.plan_morph(**dict(good, **kw))
    for kw, match in ((dict(seamless=-0.01), 'seamless'), (dict(seamless=1.01), 'seamless'), (dict(seamless=float('nan')), 'seamless'),
                      (dict(seamless=float('inf')), 'seamless'), (dict(seamless=[0.1] * 3), 'seamless'), (dict(seamless=[[0.1, 0.2]]), 'seamless'),
                      (dict(ring=15), 'ring'), (dict(ring=257), 'ring'), (dict(ring=0), 'ring'), (dict(ring=-128), 'ring'), (dict(ring=64.0), 'ring'),
                      (dict(ring=None), 'ring'), (dict(ring=True), 'ring'), (dict(ring='128'), 'ring')):
        for mask in ('hull', None):                                          # refused whether or not the mask is asked for
            with pytest.raises(ValueError, match=match):
                MP.plan_morph(**dict(good, mask=mask, **kw))
    d = MP.seam_dirs(16)
    assert d.dtype == F64 and d.shape == (16, 2) and np.array_equal(d, SR.dirs(16)) and d[0].tolist() == [1.0, 0.0]
    assert np.allclose(d[4], [0.0, 1.0], atol=1e-15), 'sample B / 4 points along +x: (uy, ux) = (cos, sin)'
    # PhotoMorph: the fields, their defaults for a caller of the earlier signature, and seam_field on host arrays
    pm = MP.PhotoMorph(None, None, None, np.zeros((2, 5)), np.zeros((2, 5)), None, None, None, None, [0, 1], [1, 0], 0.0, 2)
    assert pm.seamless is None and pm.ring is None and pm.seam_ring is None and pm.seam_diff is None and pm.seam_flags is None
    with pytest.raises(ValueError, match='seamless'):
        pm.seam_field(0)
    rng = np.random.RandomState(2)
    ring = (np.array([12.0, 15.0]) + 9.0 * SR.dirs(16) * rng.uniform(0.7, 1.0, (16, 1))).astype(F32)
    diff = rng.uniform(-50, 50, (16, 3)).astype(F32)
    rows = np.array([(0, 3, 5, 27, 36)], np.int32)
    pm = MP.PhotoMorph(None, None, None, rows, rows, None, None, None, None, [0], [1], 0.0, 2, seamless=[1.0], ring=16, seam_ring=ring[None],
                       seam_diff=diff[None], seam_flags=np.zeros(1, np.int32))
    f = pm.seam_field(0)
    rr, cc = np.divmod(np.arange(24 * 31), 31)
    assert f.dtype == F32 and f.shape == (24, 31, 3) and np.array_equal(f.reshape(-1, 3), SR.field(ring, diff, rr, cc, F32)), 'bit for bit'
    assert np.abs(f[12, 15] - SR.field(ring, diff, [12], [15], F64)[0]).max() < 1e-3 and f[0, 0].tolist() == [0.0, 0.0, 0.0]


def test_generate_script_parses_the_seamless_arguments(capsys):
    spec = importlib.util.spec_from_file_location('generate_script', os.path.join(ROOT, 'scripts', 'generate.py'))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    need = ['--configs', 'c.yaml', '--checkpoint', 'm.pt', '--appearance-dir', 'photos']
    args = script.build_parser().parse_args(need + ['--morph', '--mask', 'hull'])
    assert args.seamless is None and args.ring is None
    args = script.build_parser().parse_args(need + ['--morph', '--mask', 'hull', '--seamless', '0.75', '--ring', '64'])
    assert (args.mask, args.seamless, args.ring) == ('hull', 0.75, 64)
    for bad in (['--seamless'], ['--seamless', 'all'], ['--ring', '64.5'], ['--ring']):
        with pytest.raises(SystemExit):
            script.build_parser().parse_args(need + ['--morph'] + bad)
    capsys.readouterr()
    assert '--seamless A' in script.__doc__ and '--ring B' in script.__doc__


# ----------------------------------------------------------------------------------------------------------------------------
# the ring
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', SR.RINGS)
@pytest.mark.parametrize('K,m', SR.KERNEL_SHAPES)
def test_ring_properties(K, m, B):
    """On the GPU test's case: every ring point of a row without a flag lies on or inside every line of the region within rounding (f32
    points against f32 lines: 1e-4 pixels) and ON one of them; the points are in angular order about the centroid (every cross product
    of neighbours is > 0: the stated orientation); the row whose hull leaves its box has samples on the box's sides; the row whose
    centroid lies outside its box has bit 0 (and bit 1: the rays towards the side it lies beyond have t < 0), the NaN row is flagged and
    both hold their centroid in every sample."""
    case, poses, ca, cb, ctrl, edges, hflags = SR.fitted_case(K, m)
    rows, n = case[1], len(case[1])
    ring, flags = SR.ring_f64(poses, rows, edges, hflags, SR.dirs(B))
    assert ring.dtype == F32 and flags.dtype == np.int32
    assert flags[SR.OUTSIDE_ROW] & 1 and not hflags[SR.OUTSIDE_ROW] and flags[SR.NAN_ROW] & 1 and hflags[SR.NAN_ROW]
    assert not flags[[b for b in range(n) if b not in (SR.OUTSIDE_ROW, SR.NAN_ROW)]].any()
    for b in range(n):
        H, W = int(rows[b, 3] - rows[b, 1]), int(rows[b, 4] - rows[b, 2])
        cy, cx = ((poses[b].astype(F64) + 1) * (0.5 * np.array([H, W]))).mean(axis=0)
        if flags[b]:
            assert np.array_equal(ring[b].view(np.uint32), np.tile(ring[b, :1], (B, 1)).view(np.uint32)), 'one point, B times'
            assert np.isnan(ring[b, 0, 1]) if b == SR.NAN_ROW else np.allclose(ring[b, 0], [cy, cx], rtol=1e-6)
            continue
        lines = np.concatenate([edges[b].astype(F64), [(1, 0, 0), (-1, 0, H - 1), (0, 1, 0), (0, -1, W - 1)]])
        live = lines[np.isfinite(lines[:, 2])]
        s = live[:, 0][None, :] * ring[b, :, 0].astype(F64)[:, None] + live[:, 1][None, :] * ring[b, :, 1].astype(F64)[:, None] + live[:, 2][None, :]
        assert s.min() > -1e-4 and np.abs(s.min(axis=1)).max() < 1e-4, (b, s.min(), np.abs(s.min(axis=1)).max())
        py, px = ring[b, :, 0].astype(F64) - cy, ring[b, :, 1].astype(F64) - cx
        cr = py * np.roll(px, -1) - px * np.roll(py, -1)
        assert (cr > 0).all(), (b, 'angular order, in the stated orientation')
        assert np.abs((np.arctan2(px, py) - 2 * np.pi * np.arange(B) / B + np.pi) % (2 * np.pi) - np.pi).max() < 1e-5, 'sample s lies along dirs[s]'
    if K >= 10:
        r = ring[SR.SIDES_ROW]
        H, W = int(rows[SR.SIDES_ROW, 3] - rows[SR.SIDES_ROW, 1]), int(rows[SR.SIDES_ROW, 4] - rows[SR.SIDES_ROW, 2])
        on_side = (np.abs(r[:, 0]) < 1e-4) | (np.abs(r[:, 0] - (H - 1)) < 1e-4) | (np.abs(r[:, 1]) < 1e-4) | (np.abs(r[:, 1] - (W - 1)) < 1e-4)
        assert on_side.sum() >= B // 4, 'the side lines bind'


def test_ring_of_a_square_by_hand():
    """The flat case's square, corners (4.5, 4.5) .. (27.5, 27.5) about the centroid (16, 16) in a 32 x 32 box, grow = 1, B = 16: sample 0
    runs along +y to (27.5, 16), sample 4 along +x to (16, 27.5), sample 8 to (4.5, 16), sample 12 to (16, 4.5), the samples at 45 degrees
    are the corners, and sample 1 (22.5 degrees) meets the side y = 27.5 at x = 16 + 11.5 tan(22.5 deg)."""
    _photo, _donor, rows, _drows, poses = SR.flat_case()
    edges, hflags = HR.hull_fit(poses, rows, np.ones(1, F32))
    ring, flags = SR.ring_f64(poses, rows, edges, hflags, SR.dirs(16))
    assert flags.tolist() == [0] and hflags.tolist() == [0]
    assert ring[0, [0, 4, 8, 12]].tolist() == [[27.5, 16.0], [16.0, 27.5], [4.5, 16.0], [16.0, 4.5]]
    assert ring[0, [2, 6, 10, 14]].tolist() == [[27.5, 27.5], [4.5, 27.5], [4.5, 4.5], [27.5, 4.5]]
    assert ring[0, 1, 0] == 27.5 and abs(float(ring[0, 1, 1]) - (16 + 11.5 * np.tan(np.pi / 8))) < 2e-6
    # grown twice the square leaves the box: the sides [0, 31] bind
    edges, hflags = HR.hull_fit(poses, rows, np.full(1, 2.0, F32))
    ring, flags = SR.ring_f64(poses, rows, edges, hflags, SR.dirs(16))
    assert flags.tolist() == [0] and ring[0, [0, 4, 8, 12]].tolist() == [[31.0, 16.0], [16.0, 31.0], [0.0, 16.0], [16.0, 0.0]]
    # a box of one pixel row: the region [0, 0] x [0, 31] has no inside, the centroid is not strictly inside it
    one = np.array([(0, 4, 20, 5, 52)], np.int32)
    edges, hflags = HR.hull_fit(poses, one, np.ones(1, F32))
    assert SR.ring_f64(poses, one, edges, hflags, SR.dirs(16))[1][0] & 1


# ----------------------------------------------------------------------------------------------------------------------------
# the coordinates
# ----------------------------------------------------------------------------------------------------------------------------
def _polygon_area(ring):
    y, x = ring[:, 0].astype(F64), ring[:, 1].astype(F64)
    return 0.5 * abs(float((y * np.roll(x, -1) - x * np.roll(y, -1)).sum()))


def test_mean_value_coordinates_in_f64():
    """Inside the ring's polygon the weights are >= 0 and, normalised, sum to 1; a field that is linear on the ring comes back linear:
    mean-value coordinates have linear precision on the polygon they are given, so what is left is rounding alone, at every B (printed,
    with the same in f32).  What B does change is how much of the region the inscribed polygon covers (printed against B = 4096)."""
    case, poses, ca, cb, ctrl, edges, hflags = SR.fitted_case(64, 4)
    rows, b = case[1], 0
    H, W = int(rows[b, 3] - rows[b, 1]), int(rows[b, 4] - rows[b, 2])
    full = _polygon_area(SR.ring_f64(poses[[b]], rows[[b]], edges[[b]], hflags[[b]], SR.dirs(4096))[0][0])
    rr, cc = (a.ravel() for a in np.meshgrid(np.arange(H), np.arange(W), indexing='ij'))
    lin = lambda y, x: np.stack([3.0 + 0.5 * y - 0.25 * x, -20.0 + 2.0 * x, 100.0 - 1.5 * y + 0.125 * x], axis=-1)
    for B in (16, 64, 128, 256):
        ring, flags = SR.ring_f64(poses[[b]], rows[[b]], edges[[b]], hflags[[b]], SR.dirs(B))
        assert not flags.any()
        ring = ring[0]
        w, ln = SR.weights(ring, rr, cc, F64)
        # strictly inside the polygon, a tenth of a pixel and more from its edges
        y, x = ring[:, 0].astype(F64), ring[:, 1].astype(F64)
        ey, ex = np.roll(y, -1) - y, np.roll(x, -1) - x
        dist = ((y[:, None] - rr[None, :]) * ex[:, None] - (x[:, None] - cc[None, :]) * ey[:, None]) / np.hypot(ey, ex)[:, None]
        inside = dist.min(axis=0) > 0.1
        assert inside.sum() > 300
        wi = w[:, inside]
        assert (wi >= 0).all() and (wi.sum(axis=0) > 0).all()
        lam = wi / wi.sum(axis=0)
        assert np.abs(lam.sum(axis=0) - 1.0).max() < 1e-14
        diff = lin(y, x).astype(F32)                                          # a linear field sampled on the ring (rounded to f32, as diff is)
        want = lin(rr[inside].astype(F64), cc[inside].astype(F64))
        e64 = np.abs(SR.field(ring, diff, rr[inside], cc[inside], F64) - want).max()
        e32 = np.abs(SR.field(ring, diff, rr[inside], cc[inside], F32) - want).max()
        area = _polygon_area(ring)
        print('\nSEAM linear field B=%d: max error %.3g in f64, %.3g in f32 (values up to %.0f) over %d pixels; the ring\'s polygon covers '
              '%.2f %% of the region' % (B, e64, e32, np.abs(want).max(), int(inside.sum()), 100.0 * area / full))
        assert e64 < 1e-4 and e32 < 2e-2, 'f32 rounding of the ring values (6e-6 of 100) and of the sums'
        assert 0.9 < area / full <= 1.0 + 1e-9 and (B < 128 or area / full > 0.999)
        # the coordinates' own limit: a place ON a sample returns that sample's diff
        at = SR.field(ring, diff, [ring[3, 0]], [ring[3, 1]], F32)
        assert np.array_equal(at[0], diff[3])


# ----------------------------------------------------------------------------------------------------------------------------
# the flat-photo known answer, through the restatements
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', SR.RINGS)
def test_flat_photos_come_back_bit_for_bit(B):
    """Consequence (c): two flat photos of colours A and B, the swap (shape = 0, texture = 1) at seamless = 1: every diff is the integer
    triple A - B (A - (B + 7) with the gain (1, 7)), the membrane is that triple within rounding, and the photo comes back bit for bit at
    every weight of the soft mask and of the edge ramp; at seamless = 0 the same call changes pixels; at seamless = 0.5 half the step
    is left."""
    photo, donor, rows, drows, poses = SR.flat_case()
    edges, hflags = HR.hull_fit(poses, rows, np.ones(1, F32))
    ring, flags = SR.ring_f64(poses, rows, edges, hflags, SR.dirs(B))
    assert not flags.any() and not hflags.any()
    coef_a, coef_b, ctrl, fflags, _cond = R.fit2_f64(poses, poses, R.blend_f32(poses, poses, [0.0]), 2, 0.0)
    assert not fflags.any() and not coef_a.any() and not coef_b.any()
    one, soft = np.ones(1, F32), HR.inv_soft(rows, 0.1)
    for gain, step in ((None, (110, -13, -41)), (np.tile(np.array([1.0, 7.0], F32), (1, 3, 1)), (103, -20, -48))):
        d32 = SR.diff_f32([photo], rows, [donor], drows, ctrl, coef_a, coef_b, one, ring, flags, gain)
        d64 = SR.diff_f64([photo], rows, [donor], drows, ctrl, coef_a, coef_b, one, ring, flags, gain)
        assert (d32 == np.array(step, F32)).all() and (d64 == np.array(step, F64)).all()
        for feather in SR.FEATHERS:
            ramp = WR.inv_ramp(rows, feather)
            for fn in (SR.morph_seam_f32, SR.morph_seam_f64):
                out, cov = fn([photo], rows, [donor], drows, ctrl, coef_a, coef_b, one, ramp, edges, soft, ring, d32, one, gain)
                assert np.array_equal(out[0], photo) and cov[0].sum() == 23 * 23, (fn.__name__, feather)
                plain, _c = fn([photo], rows, [donor], drows, ctrl, coef_a, coef_b, one, ramp, edges, soft, ring, d32, 0 * one, gain)
                hull, _c = (HR.morph_f32 if fn is SR.morph_seam_f32 else HR.morph_f64)([photo], rows, [donor], drows, ctrl, coef_a, coef_b, one,
                                                                                       ramp, edges, soft, gain)
                assert np.array_equal(plain[0], hull[0]) and (plain[0] != photo).any(axis=2).sum() == 23 * 23, 'seamless = 0: the hull morph'
                half, _c = fn([photo], rows, [donor], drows, ctrl, coef_a, coef_b, one, ramp, edges, soft, ring, d32, 0.5 * one, gain)
                mid = half[0][20, 36].astype(int) - photo[20, 36]              # the middle of the box: every weight is 1
                assert np.abs(mid + 0.5 * np.array(step)).max() <= 0.5, (mid, step)


# ----------------------------------------------------------------------------------------------------------------------------
# the cap, on the restatements alone
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', SR.RINGS)
@pytest.mark.parametrize('K,m', SR.KERNEL_SHAPES)
def test_f32_restatement_against_f64(K, m, B):
    """The GPU test's case at mask_feather 0.1, feather 0 and 0.125, with and without colour_reference-style gains: morph_seam_f32
    against morph_seam_f64, both driven by the f32-rounded coefficients, the restatement's lines and ring and the f32 diffs, stays
    within unalign_reference.within_cap (one grey level, 0.5 % of the pixels with w > 0), and the two agree on which pixels have w > 0.
    Found: 0 of 1 867 (K = 3), 0 of 4 867 (K = 10) and 0 to 3 of 5 731 (K = 64) such pixels differ, by one grey level.  The flagged rows
    get the bytes of the hull morph, and so does the row with seamless = 0."""
    case, poses, ca, cb, ctrl, edges, hflags = SR.fitted_case(K, m)
    photos, rows, donors, drows, mu_a, mu_b, shape, texture, grow, seamless = case
    n = len(rows)
    ring, flags = SR.ring_f64(poses, rows, edges, hflags, SR.dirs(B))
    soft = HR.inv_soft(rows, SR.MASK_FEATHER)
    gains = np.stack([np.linspace(0.8, 1.2, 3 * n).reshape(n, 3), np.linspace(-20, 20, 3 * n).reshape(n, 3)], axis=2).astype(F32)
    for gain in (None, gains):
        d32 = SR.diff_f32(photos, rows, donors, drows, ctrl, ca, cb, texture, ring, flags, gain)
        d64 = SR.diff_f64(photos, rows, donors, drows, ctrl, ca, cb, texture, ring, flags, gain)
        assert d32.dtype == F32 and np.abs(d32 - d64).max() < 0.02 and np.abs(d32).max() > 20
        assert not d32[flags != 0].any() and not d32[SR.INACTIVE_ROW].any() and d32[0].any()
        for feather in SR.FEATHERS:
            ramp = WR.inv_ramp(rows, feather)
            ref32, cov32 = SR.morph_seam_f32(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp, edges, soft, ring, d32, seamless, gain)
            ref64, covered = SR.morph_seam_f64(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp, edges, soft, ring, d32, seamless, gain)
            n_diff, worst, _near, n_cov = UR.within_cap(ref32, ref64, covered, WR.no_band(photos))
            hull32, hcov = HR.morph_f32(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp, edges, soft, gain)
            moved = sum(int((a != h).any(axis=2).sum()) for a, h in zip(ref32, hull32))
            print('\nSEAM MORPH f32 vs f64 K=%d anchors=%d ring=%d feather=%g gain=%s: %d of %d pixels with w > 0 differ (max %d); %d differ '
                  'from the hull morph' % (K, m, B, feather, gain is not None, n_diff, n_cov, worst, moved))
            assert all(np.array_equal(x, y) for x, y in zip(covered, cov32)) and all(np.array_equal(x, y) for x, y in zip(covered, hcov))
            assert n_cov > 1500 and moved > 0.5 * n_cov, 'the membrane is at work'
            # rows that are flagged or have seamless = 0, alone: the bytes of the hull morph
            for b in (SR.OUTSIDE_ROW, n - 1):
                pick = [b]
                one, _c = SR.morph_seam_f32(photos, rows[pick], donors, drows[pick], ctrl[pick], ca[pick], cb[pick], texture[pick], ramp[pick],
                                            edges[pick], soft[pick], ring[pick], d32[pick], seamless[pick], None if gain is None else gain[pick])
                two, c2 = HR.morph_f32(photos, rows[pick], donors, drows[pick], ctrl[pick], ca[pick], cb[pick], texture[pick], ramp[pick],
                                       edges[pick], soft[pick], None if gain is None else gain[pick])
                assert all(np.array_equal(x, y) for x, y in zip(one, two)) and sum(int(c.sum()) for c in c2) > 50, b
