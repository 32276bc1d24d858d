"""Morph, host side (no GPU): the ABI of imm_morph_poses / imm_morph_u8 and their argument validation, the wrapper and plan_morph
refusals, blend_poses, known answers of the f64 restatement (tests/morph_reference.py), PhotoMorph.to_source / to_donor and the f32
restatement against the f64 one on the GPU test's case."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_reference as R                                                 # noqa: E402
import unalign_reference as UR                                              # noqa: E402
import warp_reference as WR                                                 # noqa: E402

from imm_amd import morphing as MP                                          # noqa: E402  (imports without a GPU)
from imm_amd import warping as WP                                           # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ----------------------------------------------------------------------------------------------------------------------------
# ABI and validation
# ----------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_morph_entry_points():
    from imm_amd import _lib as L
    assert L.ABI_VERSION >= 31
    header = open(os.path.join(ROOT, 'include', 'imm_morph.h')).read()
    assert L.symbols('imm_morph.h') == ['imm_morph_poses', 'imm_morph_u8']
    for text in ('THE RULE', 'Poses (imm_morph_poses)', 'Morph (imm_morph_u8)', 'rounded separately', 'logf', 'ONCE', 'links', 'ACTIVE',
                 'Consequences'):
        assert text in header, text
    src = open(os.path.join(ROOT, 'imm_amd', 'csrc', 'morph.hip')).read()
    assert 'fp contract(off)' in src and 'atomic' not in src.lower() and 'asm' not in src.lower()


def test_morph_entry_points_validate_their_arguments_without_a_device():
    from imm_amd import _lib as L
    lib = L.load()
    one, two, three = C.c_void_p(16), C.c_void_p(32), C.c_void_p(48)     # non-null pointers that are never read: validation comes first
    #       mu_a mu_b shape K   n  poses2 mu2 stream
    good = [one, one, one, 10, 3, two, two, None]
    bad_args = [(i, None) for i in (0, 1, 2, 5, 6)] + [(3, 0), (3, -1), (3, 81), (4, 0), (4, -1), (4, 32768)]
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert lib.imm_morph_poses(*args) == -1, (i, bad)
        assert b'morph_poses' in lib.imm_last_error()
    #       src  dst  offs hw  n_img donor doffs dhw n_donor boxes dboxes links ramp texture ctrl coef_a coef_b M  n  pixels stream
    good = [one, two, one, one, 2, three, one, one, 3, one, one, one, one, one, one, one, one, 18, 3, 100, None]
    bad_args = [(i, None) for i in (0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16)]
    bad_args += [(1, one), (5, two), (4, 0), (8, 0), (8, -1), (17, 2), (17, 81), (18, 0), (18, 65536), (19, 0), (19, -5)]
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert lib.imm_morph_u8(*args) == -1, (i, bad)
        assert b'morph_u8' in lib.imm_last_error()
    # (the donor buffer may be src itself: not refused on that ground; nothing is launched here, M is out of range)
    args = list(good)
    args[5], args[17] = one, 81
    assert lib.imm_morph_u8(*args) == -1 and b'control points' in lib.imm_last_error()


def test_wrapper_refusals_come_before_any_device_call():
    from imm_amd import ops
    z = lambda *sh, **kw: torch.zeros(*sh, **kw)           # host tensors: a wrapper that got as far as the library would fault
    n, K, M = 2, 10, 18
    mu_a, mu_b, shape, poses2, mu2 = z(n, K, 2), z(n, K, 2), z(n), z(2, n, K, 2), z(2, n, K, 2)
    for kw, match in ((dict(mu_a=z(n, K, 3)), 'mu_a'), (dict(mu_b=z(n, K + 1, 2)), 'mu_b'), (dict(mu_b=mu_b.double()), 'mu_b'),
                      (dict(shape=z(n + 1)), 'shape'), (dict(shape=z(n, 1)), 'shape'), (dict(poses2=z(2 * n, K, 2)), 'poses2'),
                      (dict(mu2=z(2, n, K, 2).transpose(0, 1)), 'mu2'), (dict(mu_a=z(n, 81, 2)), 'landmarks'),
                      (dict(mu_a=z(0, K, 2)), 'rows'), (dict(mu_a=poses2[0]), 'overlaps'), (dict(mu2=poses2), 'overlaps')):
        args = dict(mu_a=mu_a, mu_b=mu_b, shape=shape, poses2=poses2, mu2=mu2)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.morph_poses(**args)
    src, dst, don = z(64, dtype=torch.uint8), z(64, dtype=torch.uint8), z(48, dtype=torch.uint8)
    offs, hw, doffs, dhw = z(1, dtype=torch.int64), z(1, 2, dtype=torch.int32), z(2, dtype=torch.int64), z(2, 2, dtype=torch.int32)
    boxes, links, ramp, tex = z(n, 5, dtype=torch.int32), z(n, 2, dtype=torch.int32), z(n, 2), z(n)
    ctrl, coef = z(n, M, 2), z(n, M + 3, 2)
    for kw, match in ((dict(src=src.float()), 'src'), (dict(dst=src), 'copy of src'), (dict(dst=z(32, dtype=torch.uint8)), 'copy of src'),
                      (dict(donor=dst), 'never dst'), (dict(donor=don.float()), 'donor'), (dict(boxes=boxes.long()), 'boxes'),
                      (dict(donor_boxes=boxes[:1]), 'donor_boxes'), (dict(links=links[:1]), 'links'), (dict(inv_ramp=ramp.double()), 'inv_ramp'),
                      (dict(texture=z(n, 1)), 'texture'), (dict(texture=tex.double()), 'texture'), (dict(coef_a=z(n, M, 2)), 'coef_a'),
                      (dict(coef_b=z(n, M + 3, 3)), 'coef_b'), (dict(ctrl=z(n, 2, 2)), 'control points'), (dict(hw=hw.long()), 'hw'),
                      (dict(donor_hw=dhw.long()), 'donor_hw'), (dict(donor_offsets=offs), 'donor_offsets'),
                      (dict(max_box_pixels=0), 'max_box_pixels')):
        args = dict(src=src, dst=dst, offsets=offs, hw=hw, donor=don, donor_offsets=doffs, donor_hw=dhw, boxes=boxes, donor_boxes=boxes,
                    links=links, inv_ramp=ramp, texture=tex, ctrl=ctrl, coef_a=coef, coef_b=coef, max_box_pixels=9)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.morph_u8(**args)


def test_morph_paste_checks_once_and_chooses_the_entry(monkeypatch):
    """ops.morph_paste on host tensors (n = 2, M = 3, K = 1, B = 16, 64-byte buffers): what it refuses is refused before a launch, with
    a ValueError that names the argument; the named wrappers refuse a None for the arguments that define them; and with the library
    call recorded instead of made, what is given chooses the entry point, with as many arguments as _lib declares for it."""
    from imm_amd import _lib as L
    from imm_amd import ops
    z = lambda *sh, **kw: torch.zeros(*sh, **kw)
    n, M, K, B = 2, 3, 1, 16
    pool = z(512, dtype=torch.uint8)                       # dst is its head: a tensor viewed on its head overlaps dst
    over = lambda *sh: pool[:4 * int(np.prod(sh))].view(torch.float32).view(*sh)
    boxes, coef = z(n, 5, dtype=torch.int32), z(n, M + 3, 2)
    common = (z(64, dtype=torch.uint8), pool[:64], z(1, dtype=torch.int64), z(1, 2, dtype=torch.int32), z(64, dtype=torch.uint8),
              z(1, dtype=torch.int64), z(1, 2, dtype=torch.int32), boxes, boxes, z(n, 2, dtype=torch.int32), z(n, 2), z(n), z(n, M, 2), coef, coef)
    shapes = dict(gain=(n, 3, 2), edges=(n, K, 3), inv_soft=(n,), ring=(n, B, 2), diff=(n, B, 3), seamless=(n,))
    opt = {k: z(*sh) for k, sh in shapes.items()}
    pick = lambda *names, **kw: dict({k: opt[k] for k in names}, **kw)
    refused = [(pick('inv_soft'), 'edges is None'), (pick('edges'), 'inv_soft is None'),
               (pick('edges', 'inv_soft', 'ring', 'seamless'), 'diff is None'), (pick('edges', 'inv_soft', 'ring', 'diff'), 'seamless is None'),
               (pick('ring', 'diff', 'seamless'), 'edges is None'), (pick('gain', 'ring', 'diff', 'seamless'), 'edges is None'),
               (pick(gain=z(n, 3)), 'gain must be'), (pick('inv_soft', edges=z(n, 81, 3)), 'edges must be f32'),
               (pick('edges', 'inv_soft', 'seamless', ring=z(n, 15, 2), diff=z(n, 15, 3)), 'morph_seam_u8: ring must be'),
               (pick('edges', 'inv_soft', 'seamless', ring=z(n, 257, 2), diff=z(n, 257, 3)), 'morph_seam_u8: ring must be')]
    refused += [(dict(opt, **{k: over(*sh)}), '%s overlaps dst' % k) for k, sh in shapes.items()]
    for kw, match in refused:
        with pytest.raises(ValueError, match=match):
            ops.morph_paste(*common, 9, **kw)
    g, e, s_, r, d, a = (opt[k] for k in ('gain', 'edges', 'inv_soft', 'ring', 'diff', 'seamless'))
    for fn, args, match in ((ops.morph_colour_u8, (None,), 'gain'), (ops.morph_hull_u8, (g, None, s_), 'edges'),
                            (ops.morph_hull_u8, (None, e, None), 'inv_soft'), (ops.morph_seam_u8, (g, None, s_, r, d, a), 'edges'),
                            (ops.morph_seam_u8, (g, e, None, r, d, a), 'inv_soft'), (ops.morph_seam_u8, (None, e, s_, None, d, a), 'ring'),
                            (ops.morph_seam_u8, (g, e, s_, r, None, a), 'diff'), (ops.morph_seam_u8, (g, e, s_, r, d, None), 'seamless')):
        with pytest.raises(ValueError, match='%s needs %s' % (fn.__name__, match)):
            fn(*common, *args, 9)
    calls = []
    monkeypatch.setattr(ops, 'call', lambda name, *args: calls.append((name, len(args))))
    monkeypatch.setattr(ops, '_s', lambda: None)
    for kw, entry in ((pick(), 'imm_morph_u8'), (pick('gain'), 'imm_morph_colour_u8'), (pick('edges', 'inv_soft'), 'imm_morph_hull_u8'),
                      (pick('gain', 'edges', 'inv_soft'), 'imm_morph_hull_u8'), (opt, 'imm_morph_seam_u8'),
                      (pick('edges', 'inv_soft', 'ring', 'diff', 'seamless'), 'imm_morph_seam_u8')):
        ops.morph_paste(*common, 9, **kw)
        assert calls[-1] == (entry, len(L.signature(entry)[1])), kw.keys()
    ops.morph_u8(*common, 9), ops.morph_colour_u8(*common, g, 9), ops.morph_hull_u8(*common, None, e, s_, 9)
    ops.morph_seam_u8(*common, g, e, s_, r, d, a, 9)
    assert [c[0] for c in calls[-4:]] == ['imm_morph_u8', 'imm_morph_colour_u8', 'imm_morph_hull_u8', 'imm_morph_seam_u8']


# ----------------------------------------------------------------------------------------------------------------------------
# plan_morph and blend_poses
# ----------------------------------------------------------------------------------------------------------------------------
def test_plan_morph_forms_and_refusals():
    photos = [np.zeros((40, 50, 3), np.uint8), np.zeros((30, 30, 3), np.uint8)]
    donors = [np.zeros((20, 25, 3), np.uint8), np.zeros((35, 30), np.uint8)]
    K = 10
    lm_a, lm_b = R.landmarks(K, 2, np.random.RandomState(1))
    plan = MP.plan_morph(photos, donors, None, None, 0.5, None, 0.125, K)
    assert plan.rows.tolist() == [[0, 0, 0, 40, 50], [1, 0, 0, 30, 30]] and plan.donor_rows.tolist() == [[0, 0, 0, 20, 25], [1, 0, 0, 35, 30]]
    assert plan.donors[1].shape == (35, 30, 3) and plan.shape.dtype == F32 and plan.shape.tolist() == [0.5, 0.5] == plan.texture.tolist()
    assert (plan.feather, plan.anchors, plan.lam, plan.M) == (0.125, 2, 0.0, 18) and plan.landmarks is None and plan.donor_landmarks is None
    # one donor row for all faces; per-row shape and texture; given landmarks
    plan = MP.plan_morph(photos, donors[:1], [(1, 2, 2, 20, 20)] * 3, [(0, 1, 1, 11, 21)], [0.0, 0.25, 1.0], 1.0, 0.0, K, anchors=0,
                         landmarks=np.tile(lm_a[:1], (3, 1, 1)), donor_landmarks=lm_b[:1])
    assert plan.donor_rows.tolist() == [[0, 1, 1, 11, 21]] * 3 and plan.donor_rows_given.tolist() == [[0, 1, 1, 11, 21]]
    assert plan.shape.tolist() == [0.0, 0.25, 1.0] and plan.texture.tolist() == [1.0] * 3 and plan.M == 10
    assert tuple(plan.landmarks.shape) == (3, K, 2) and tuple(plan.donor_landmarks.shape) == (1, K, 2) and plan.landmarks.dtype == torch.float32
    nan = lm_a.copy()
    nan[1, 2, 0] = np.nan
    good = dict(photos=photos, donors=donors, boxes=None, donor_boxes=None, shape=0.5, texture=None, feather=0.125, K=K)
    for kw, match in ((dict(donors=donors + donors[:1]), '3 donors for 2 faces'), (dict(donor_boxes=[(0, 0, 0, 5, 5)] * 3), '3 donors for 2 faces'),
                      (dict(shape=1.5), 'shape'), (dict(shape=-0.1), 'shape'), (dict(shape=float('nan')), 'shape'),
                      (dict(shape=[0.1, 0.2, 0.3]), 'shape'), (dict(shape=[[0.1, 0.2]]), 'shape'),
                      (dict(texture=2.0), 'texture'), (dict(texture=float('inf')), 'texture'), (dict(texture=[0.5]), 'texture'),
                      (dict(feather=0.75), 'feather'), (dict(anchors=18), '<= 80 control points'), (dict(anchors=-1), 'anchors'),
                      (dict(lam=-0.1), 'lam'), (dict(lam=float('nan')), 'lam'),
                      (dict(photos=torch.zeros(2, 128, 128, 3)), 'u8 arrays'), (dict(donors=torch.zeros(2, 128, 128, 3)), 'u8 arrays'),
                      (dict(donors=[]), 'u8 arrays'), (dict(boxes=[(5, 0, 0, 5, 5)]), 'names image'),
                      (dict(donor_boxes=[(2, 0, 0, 5, 5)] * 2), 'names image'), (dict(donor_boxes=[(0, 5, 5, 5, 9)] * 2), 'empty'),
                      (dict(landmarks=lm_a[:1]), 'landmarks must be'), (dict(landmarks=lm_a[:, :9]), 'landmarks must be'),
                      (dict(donor_landmarks=lm_b[:1]), 'donor_landmarks must be'), (dict(landmarks=nan), 'landmarks must be finite'),
                      (dict(donor_landmarks=nan), 'donor_landmarks must be finite')):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            MP.plan_morph(**args)


def test_blend_poses_end_points_and_order():
    rng = np.random.RandomState(4)
    a, b = rng.uniform(-1, 1, (6, 10, 2)).astype(F32), rng.uniform(-1, 1, (6, 10, 2)).astype(F32)
    s = np.array([0.0, 1.0, 0.5, 0.37, 0.0, 1.0], dtype=F32)
    a[3, 2, 1], b[2, 0, 0] = np.nan, np.nan
    a[4, 1, 0], b[5, 3, 1] = -0.0, -0.0
    p = MP.blend_poses(a, b, s)
    assert p.dtype == F32 and p.shape == a.shape
    assert np.array_equal(p[0], a[0]) and np.array_equal(p[4], a[4]), 'shape 0 gives mu_a as a value'
    assert np.array_equal(p[1], b[1]) and np.array_equal(p[5], b[5]), 'shape 1 gives mu_b as a value'
    assert np.isnan(p[3, 2, 1]) and np.isnan(p[2, 0, 0]) and np.isnan(p).sum() == 2
    assert np.array_equal(p.view(np.uint32), R.blend_f32(a, b, s).view(np.uint32)), 'the kernel order, bit for bit'
    ok = ~np.isnan(p)
    assert np.abs(p[ok] - R.blend_f64(a, b, s)[ok]).max() <= 2.0 ** -23              # three roundings of values below 1
    # in between, the blend lies between its end points
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    assert ((p >= lo - 1e-6) & (p <= hi + 1e-6))[ok].all()
    for bad in (dict(mu_b=b[:5]), dict(shape=s[:5]), dict(mu_a=a[0])):
        args = dict(mu_a=a, mu_b=b, shape=s)
        args.update(bad)
        with pytest.raises(ValueError, match='must be'):
            MP.blend_poses(**args)


# ----------------------------------------------------------------------------------------------------------------------------
# the rule: known answers of the f64 restatement
# ----------------------------------------------------------------------------------------------------------------------------
def _one_face(seed=3, K=6):
    rng = np.random.RandomState(seed)
    photo = rng.randint(0, 256, size=(48, 56, 3)).astype(np.uint8)
    rows = np.array([(0, 4, 20, 36, 52)], dtype=np.int32)
    mu_a, mu_b = R.landmarks(K, 1, rng)
    return rng, photo, rows, mu_a, mu_b


def test_texture_zero_is_the_warp():
    for K, m in R.KERNEL_SHAPES[:2]:
        case, poses, coef_a, coef_b, ctrl, flags, _cond = R.fitted_case(K, m, 0.0)
        photos, rows, donors, drows, _a, _b, _s, _t = case
        zero = np.zeros(len(rows), F32)
        for feather in R.FEATHERS:
            ramp = WR.inv_ramp(rows, feather)
            got64, cov = R.morph_f64(photos, rows, donors, drows, ctrl, coef_a, coef_b, zero, ramp)
            got32, cov32 = R.morph_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, zero, ramp)
            # warp_f64 knows no donors: the row without a donor photo is taken out of its rows
            live = rows.copy()
            live[R.BAD_DONOR_ROW, 0] = -1
            want64, wcov = WR.warp_f64(photos, live, ctrl, coef_a, ramp)
            want32 = WR.warp_f32(photos, live, ctrl, coef_a, ramp)
            assert all(np.array_equal(x, y) for x, y in zip(got64, want64)) and all(np.array_equal(x, y) for x, y in zip(cov, wcov))
            assert all(np.array_equal(x, y) for x, y in zip(got32, want32)) and all(np.array_equal(x, y) for x, y in zip(cov32, wcov))


def test_constant_donor_fills_the_box():
    rng, photo, rows, mu_a, mu_b = _one_face()
    donor = np.empty((30, 20, 3), np.uint8)
    donor[:] = (200, 17, 99)
    drows = np.array([(0, -3, 2, 25, 30)], dtype=np.int32)
    poses = R.blend_f32(mu_a, mu_b, [0.5])
    coef_a, coef_b, ctrl, flags, _cond = R.fit2_f64(mu_a, mu_b, poses, 2, 0.0)
    assert not flags.any()
    for fn in (R.morph_f64, R.morph_f32):
        out, cov = fn([photo], rows, [donor], drows, ctrl, coef_a, coef_b, [1.0], WR.inv_ramp(rows, 0.0))
        assert cov[0].sum() == 32 * 32 and (out[0][4:36, 20:52] == (200, 17, 99)).all()
        assert np.array_equal(out[0][~cov[0]], photo[~cov[0]])


def test_shifted_donor_returns_the_photo():
    """The donor is the photo shifted by whole pixels, the donor box is the box shifted alike and mu_b = mu_a: both splines are the same,
    both samples are the same pixels' and every texture returns what the warp alone gives; with shape 0 on top, the photo itself."""
    rng, photo, rows, mu_a, _mu_b = _one_face()
    dy, dx = 5, -7
    donor = np.zeros((60, 70, 3), np.uint8)
    donor[dy + 2:dy + 2 + 48, dx + 9:dx + 9 + 56] = photo                # donor[r + 7, c + 2] = photo[r, c]
    drows = rows + np.array([0, 7, 2, 7, 2], dtype=np.int32)
    ident = R.fit2_f64(mu_a, mu_a, mu_a, 2, 0.0)
    assert not ident[0].any() and not ident[1].any(), 'a zero right-hand side gives zero coefficients'
    for texture in (0.0, 0.37, 1.0):
        for feather in R.FEATHERS:
            ramp = WR.inv_ramp(rows, feather)
            for fn in (R.morph_f64, R.morph_f32):
                out, cov = fn([photo], rows, [donor], drows, ident[2], ident[0], ident[1], [texture], ramp)
                assert np.array_equal(out[0], photo) and cov[0].sum() == 32 * 32, (texture, feather, fn.__name__)
    # a real warp on both sides: target poses away from mu_a, both splines lead to the same pixels
    poses = (mu_a + rng.normal(0, 0.04, mu_a.shape)).astype(F32)
    coef_a, coef_b, ctrl, flags, _cond = R.fit2_f64(mu_a, mu_a, poses, 2, 0.0)
    assert np.array_equal(coef_a, coef_b) and coef_a.any()
    ramp = WR.inv_ramp(rows, 0.125)
    want, _c = WR.warp_f64([photo], rows, ctrl, coef_a, ramp)
    for texture in (0.0, 0.37, 1.0):
        out, _c = R.morph_f64([photo], rows, [donor], drows, ctrl, coef_a, coef_b, [texture], ramp)
        # the donor sample sits at the same place up to the rounding of q -> pixels: at most one grey level on a pixel or two
        d = np.abs(out[0].astype(int) - want[0].astype(int))
        assert d.max() <= 1 and (d > 0).sum() <= 3, (texture, int(d.max()), int((d > 0).sum()))


def test_identity_on_a_noise_photo_bit_for_bit():
    """Zero coefficients on both sides, donor buffer, photo and box equal to the row's own: the photo returns bit for bit from the f32
    restatement for every texture and feather (odd box sizes, boxes over the photo's edges)."""
    rng = np.random.RandomState(11)
    photo = rng.randint(0, 256, size=(70, 93, 3)).astype(np.uint8)
    rows = np.array([(0, 3, 5, 64, 82), (0, -9, 40, 28, 101), (0, 30, -4, 77, 33), (0, 10, 10, 11, 57)], dtype=np.int32)
    n, M = len(rows), 18
    ctrl = WP.control_points(R.landmarks(10, n, rng)[0], 2)
    zero = np.zeros((n, M + 3, 2), F32)
    for texture in (0.0, 0.37, 1.0):
        for feather in R.FEATHERS:
            out, cov = R.morph_f32([photo], rows, [photo], rows, ctrl, zero, zero, np.full(n, texture, F32), WR.inv_ramp(rows, feather))
            assert np.array_equal(out[0], photo) and cov[0].sum() > 5000, (texture, feather)


# ----------------------------------------------------------------------------------------------------------------------------
# PhotoMorph
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', [0, 2])
def test_photo_morph_maps(m):
    """At lam = 0 the blended landmarks, in the pixels of the face's box, map to the face's own landmarks in its photo (to_source) and
    to the donor's landmarks in the pixels of the donor box (to_donor); the anchors map to the border of either box."""
    K, n = 10, 3
    rng = np.random.RandomState(2)
    mu_a, mu_b = R.landmarks(K, n, rng)
    shape = np.array([0.3, 0.0, 1.0], dtype=F32)
    rows = np.array([(0, 10, 20, 110, 140), (1, -5, -5, 60, 45), (0, 0, 0, 33, 77)], dtype=np.int32)
    drows = np.array([(1, 4, 4, 84, 64), (0, 10, 0, 40, 90), (0, -8, 3, 41, 52)], dtype=np.int32)
    poses = MP.blend_poses(mu_a, mu_b, shape)
    coef_a, coef_b, ctrl, flags, _cond = R.fit2_f64(mu_a, mu_b, poses, m, 0.0)
    assert not flags.any()
    px = lambda q, rw: rw[:, None, 1:3].astype(np.float64) + (np.asarray(q, np.float64) + 1.0) * ((rw[:, None, 3:5] - rw[:, None, 1:3]) / 2.0)
    for ca, cb, tol in ((coef_a, coef_b, 1e-9), (coef_a.astype(F32), coef_b.astype(F32), 1e-4)):
        pm = MP.PhotoMorph(ca, cb, ctrl, rows, drows, mu_a, mu_b, poses, flags, shape, shape, 0.0, m)
        src, don = pm.to_source(px(poses, rows)), pm.to_donor(px(poses, rows))
        assert src.shape == (n, K, 2) and src.dtype == np.float64 and don.shape == (n, K, 2)
        assert np.abs(src - px(mu_a, rows)).max() < tol and np.abs(don - px(mu_b, drows)).max() < tol
        if m:
            ring = np.broadcast_to(WP.warp_anchors(m)[None], (n, 4 * m, 2))
            assert np.abs(pm.to_source(px(ring, rows)) - px(ring, rows)).max() < tol
            assert np.abs(pm.to_donor(px(ring, rows)) - px(ring, drows)).max() < tol
        # against the formulas, point by point
        pts = rng.uniform(0, 100, (n, 7, 2))
        for b in range(n):
            half, dhalf = (rows[b, 3:5] - rows[b, 1:3]) / 2.0, (drows[b, 3:5] - drows[b, 1:3]) / 2.0
            q = (pts[b] - rows[b, 1:3]) / half - 1.0
            assert np.allclose(pm.to_source(pts)[b], pts[b] + half * WP.displacement(ca[b], ctrl[b], q), rtol=0, atol=1e-9)
            assert np.allclose(pm.to_donor(pts)[b], drows[b, 1:3] + (q + WP.displacement(cb[b], ctrl[b], q) + 1.0) * dhalf, rtol=0, atol=1e-9)
    assert (pm.lam, pm.anchors) == (0.0, m) and pm.shape.dtype == F32 and pm.rows.dtype == np.int32
    for fn in (pm.to_source, pm.to_donor):
        with pytest.raises(ValueError, match='points_px'):
            fn(np.zeros((2, 4, 2)))
    # rows 1 and 2: shape 0 and 1, one of the two maps is the plain box-to-box map
    pts = rng.uniform(0, 60, (n, 5, 2))
    exact = MP.PhotoMorph(coef_a, coef_b, ctrl, rows, drows, mu_a, mu_b, poses, flags, shape, shape, 0.0, m)
    assert np.array_equal(exact.to_source(pts)[1], pts[1]) and not coef_b[2].any()


# ----------------------------------------------------------------------------------------------------------------------------
# the f32 restatement against the f64 one on the GPU test's case
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,m', R.KERNEL_SHAPES)
def test_f32_restatement_against_f64(K, m):
    """The committed seed: morph_f32 against morph_f64, both driven by the f32-rounded coefficients, differs by at most one grey level on
    at most HALF the cap's share (0.25 % of the covered pixels), for every lam and feather of the GPU parity test: the other half is left
    to the device's log.  The condition numbers of the systems stay <= 1e4."""
    for lam in R.LAMS:
        case, poses, coef_a, coef_b, ctrl, flags, cond = R.fitted_case(K, m, lam)
        photos, rows, donors, drows, mu_a, mu_b, shape, texture = case
        good = np.nonzero(flags == 0)[0]
        assert flags.tolist() == [int(b == R.NAN_ROW) for b in range(len(rows))]
        print('\nMORPH FIT K=%d anchors=%d lam=%g: condition numbers %.3g .. %.3g' % (K, m, lam, cond[good].min(), cond[good].max()))
        assert cond[good].max() <= 1e4
        assert np.array_equal(poses, MP.blend_poses(mu_a, mu_b, shape)) or np.isnan(poses).any()
        assert np.array_equal(poses[good], MP.blend_poses(mu_a, mu_b, shape)[good])
        assert np.array_equal(poses[R.SHAPE_ZERO_ROW], mu_a[R.SHAPE_ZERO_ROW]) and np.array_equal(poses[R.SHAPE_ONE_ROW], mu_b[R.SHAPE_ONE_ROW])
        assert not coef_a[R.SHAPE_ZERO_ROW].any() and not coef_b[R.SHAPE_ONE_ROW].any()
        ca, cb = coef_a.astype(F32), coef_b.astype(F32)
        for feather in R.FEATHERS:
            ramp = WR.inv_ramp(rows, feather)
            ref64, covered = R.morph_f64(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp)
            ref32, cov32 = R.morph_f32(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp)
            n_diff, worst, _near, n_cov = UR.within_cap(ref32, ref64, covered, WR.no_band(photos))
            print('MORPH f32 vs f64 K=%d anchors=%d lam=%g feather=%g: %d of %d covered pixels differ (max %d)' % (
                K, m, lam, feather, n_diff, n_cov, worst))
            assert n_diff <= 0.0025 * n_cov
            assert all(np.array_equal(x, y) for x, y in zip(covered, cov32))
            # what no row covers is the input's; the rows that write nothing cover nothing
            for p, o, cov in zip(photos, ref32, covered):
                assert np.array_equal(o[~cov], p[~cov])
            assert not covered[3].any() and n_cov > 1500
            y0, x0, y1, x1 = rows[R.NAN_ROW, 1:]
            assert not covered[rows[R.NAN_ROW, 0]][y0:y1, x0:x1].any()
            changed = sum(int((o != p).any(axis=2).sum()) for o, p in zip(ref32, photos))
            assert changed > 0.3 * n_cov, 'the morph moves pixels'
    # the row without a donor photo writes nothing although its own box is valid: alone, it returns the photos
    one = slice(R.BAD_DONOR_ROW, R.BAD_DONOR_ROW + 1)
    out, cov = R.morph_f32(photos, rows[one], donors, drows[one], ctrl[one], ca[one], cb[one], texture[one], WR.inv_ramp(rows[one], 0.125))
    assert all(np.array_equal(a, b) for a, b in zip(out, photos)) and not any(c.any() for c in cov)
