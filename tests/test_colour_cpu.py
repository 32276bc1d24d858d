"""Colour matching, host side (no GPU): the ABI of imm_colour_stats_u8 / imm_colour_gain / imm_morph_colour_u8 and their argument
validation, the wrapper and plan_morph refusals, the integer ellipse of the restatement (tests/colour_reference.py) against a float64
one, hand-derived known answers of the gain rule, and the f32 restatement of the morph with colour against the f64 one on the GPU
test's case."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colour_reference as CO                                               # noqa: E402
import morph_reference as R                                                 # noqa: E402
import unalign_reference as UR                                              # noqa: E402
import warp_reference as WR                                                 # noqa: E402

from imm_amd import morphing as MP                                          # noqa: E402  (imports without a GPU)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAMES = ['imm_colour_gain', 'imm_colour_stats_u8', 'imm_morph_colour_u8']


# ----------------------------------------------------------------------------------------------------------------------------
# ABI and validation
# ----------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_colour_entry_points():
    from imm_amd import _lib as L
    assert L.ABI_VERSION >= 32
    header = open(os.path.join(ROOT, 'include', 'imm_colour.h')).read()
    assert L.symbols('imm_colour.h') == NAMES
    for text in ('THE RULE', 'Region.', 'Statistics (imm_colour_stats_u8)', 'Gain (imm_colour_gain)', 'Morph with colour (imm_morph_colour_u8)',
                 'rounded separately', 'in 64 bits', 'Consequences', 'exactly (1, 0)', 'x / x = 1'):
        assert text in header, text
    src = open(os.path.join(ROOT, 'imm_amd', 'csrc', 'colour.hip')).read()
    assert 'fp contract(off)' in src and src.count('atomicAdd(') == 1 and 'asm' not in src.lower()
    morph = open(os.path.join(ROOT, 'imm_amd', 'csrc', 'morph.hip')).read()
    assert 'imm_morph_colour_u8' in morph and 'morph_u8_kernel<true>' in morph and 'morph_u8_kernel<false>' in morph


def test_colour_entry_points_validate_their_arguments_without_a_device():
    from imm_amd import _lib as L
    lib = L.load()
    one, two, three = C.c_void_p(16), C.c_void_p(32), C.c_void_p(48)     # non-null pointers that are never read: validation comes first
    #       buf  offs hw  n_img boxes n  pixels sums stream
    good = [one, one, one, 2, one, 3, 100, two, None]
    bad_args = [(i, None) for i in (0, 1, 2, 4, 7)] + [(3, 0), (3, -1), (5, 0), (5, -1), (5, 65536), (6, 0), (6, -7)]
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert lib.imm_colour_stats_u8(*args) == -1, (i, bad)
        assert b'colour_stats_u8' in lib.imm_last_error()
    #       sums_a sums_b amount max_gain n gain flags stream
    good = [one, one, one, 2.0, 3, two, three, None]
    bad_args = [(i, None) for i in (0, 1, 2, 5, 6)] + [(3, 0.5), (3, 0.0), (3, -2.0), (3, float('inf')), (3, float('nan')), (4, 0), (4, -1),
                                                      (4, 65536)]
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert lib.imm_colour_gain(*args) == -1, (i, bad)
        assert b'colour_gain' in lib.imm_last_error()
    #       src  dst  offs hw  n_img donor doffs dhw n_donor boxes dboxes links ramp texture ctrl coef_a coef_b gain M  n  pixels stream
    good = [one, two, one, one, 2, three, one, one, 3, one, one, one, one, one, one, one, one, one, 18, 3, 100, None]
    bad_args = [(i, None) for i in (0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17)]
    bad_args += [(1, one), (5, two), (4, 0), (8, 0), (8, -1), (18, 2), (18, 81), (19, 0), (19, 65536), (20, 0), (20, -5)]
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert lib.imm_morph_colour_u8(*args) == -1, (i, bad)
        assert b'morph_colour_u8' in lib.imm_last_error()
    # imm_morph_u8 shares these checks with it now: the same refusals under its own name
    good = good[:17] + good[18:]
    bad_args = [(i, None) for i in (0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16)]
    bad_args += [(1, one), (5, two), (4, 0), (8, 0), (8, -1), (17, 2), (17, 81), (18, 0), (18, 65536), (19, 0), (19, -5)]
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert lib.imm_morph_u8(*args) == -1, (i, bad)
        assert b'morph_u8: ' in lib.imm_last_error() and b'colour' not in lib.imm_last_error()


def test_wrapper_refusals_come_before_any_device_call():
    from imm_amd import ops
    z = lambda *sh, **kw: torch.zeros(*sh, **kw)           # host tensors: a wrapper that got as far as the library would fault
    n, M = 2, 18
    buf, offs, hw = z(64, dtype=torch.uint8), z(1, dtype=torch.int64), z(1, 2, dtype=torch.int32)
    boxes, sums = z(n, 5, dtype=torch.int32), z(n, 7, dtype=torch.int64)
    for kw, match in ((dict(buf=buf.float()), 'buf'), (dict(hw=hw.long()), 'hw'), (dict(hw=hw[:0]), 'at least one image'),
                      (dict(offsets=z(2, dtype=torch.int64)), 'offsets'), (dict(boxes=boxes.long()), 'boxes'), (dict(boxes=boxes[:0]), 'rows'),
                      (dict(boxes=z(n, 4, dtype=torch.int32)), 'boxes'), (dict(sums=z(n, 7)), 'sums'), (dict(sums=sums[:1]), 'sums'),
                      (dict(sums=z(7, n, dtype=torch.int64).t()), 'sums'), (dict(max_box_pixels=0), 'max_box_pixels')):
        args = dict(buf=buf, offsets=offs, hw=hw, boxes=boxes, max_box_pixels=9, sums=sums)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.colour_stats_u8(**args)
    amount, gain, flags = z(n), z(n, 3, 2), z(n, dtype=torch.int32)
    for kw, match in ((dict(sums_a=sums.int()), 'sums_a'), (dict(sums_b=sums[:1]), 'sums_b'), (dict(amount=z(n, 1)), 'amount'),
                      (dict(amount=amount.double()), 'amount'), (dict(gain=z(n, 2, 3)), 'gain'), (dict(flags=flags.long()), 'flags'),
                      (dict(sums_a=sums[:0]), 'rows'), (dict(max_gain=0.99), 'max_gain'), (dict(max_gain=float('inf')), 'max_gain'),
                      (dict(max_gain=float('nan')), 'max_gain')):
        args = dict(sums_a=sums, sums_b=sums, amount=amount, max_gain=2.0, gain=gain, flags=flags)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.colour_gain(**args)
    src, dst, don = z(64, dtype=torch.uint8), z(64, dtype=torch.uint8), z(48, dtype=torch.uint8)
    doffs, dhw = z(2, dtype=torch.int64), z(2, 2, dtype=torch.int32)
    links, ramp, tex, ctrl, coef = z(n, 2, dtype=torch.int32), z(n, 2), z(n), z(n, M, 2), z(n, M + 3, 2)
    for kw, match in ((dict(gain=z(n, 3)), 'gain'), (dict(gain=gain.double()), 'gain'), (dict(gain=z(n + 1, 3, 2)), 'gain'),
                      (dict(dst=src), 'copy of src'), (dict(donor=dst), 'never dst'), (dict(texture=z(n, 1)), 'texture'),
                      (dict(ctrl=z(n, 2, 2)), 'morph_colour_u8 serves'), (dict(coef_b=z(n, M + 3, 3)), 'coef_b'),
                      (dict(max_box_pixels=0), 'max_box_pixels')):
        args = dict(src=src, dst=dst, offsets=offs, hw=hw, donor=don, donor_offsets=doffs, donor_hw=dhw, boxes=boxes, donor_boxes=boxes,
                    links=links, inv_ramp=ramp, texture=tex, ctrl=ctrl, coef_a=coef, coef_b=coef, gain=gain, max_box_pixels=9)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.morph_colour_u8(**args)


def test_plan_morph_checks_colour_and_max_gain():
    photos = [np.zeros((40, 50, 3), np.uint8), np.zeros((30, 30, 3), np.uint8)]
    donors = [np.zeros((20, 25, 3), np.uint8), np.zeros((35, 30), np.uint8)]
    K = 10
    good = dict(photos=photos, donors=donors, boxes=None, donor_boxes=None, shape=0.5, texture=None, feather=0.125, K=K)
    plan = MP.plan_morph(**good)
    assert len(vars(plan)) == 21 and plan.colour.dtype == F32 and plan.colour.tolist() == [0.0, 0.0] and plan.max_gain == 2.0
    plan = MP.plan_morph(colour=[0.25, 1.0], max_gain=3, **good)
    assert plan.colour.tolist() == [0.25, 1.0] and plan.max_gain == 3.0 and isinstance(plan.max_gain, float)
    assert MP.plan_morph(colour=1, max_gain=1.0, **good).colour.tolist() == [1.0, 1.0]
    huge = [(0, -40000, -40000, 40000, 40000), (1, 0, 0, 30, 30)]                      # 6.4e9 pixels
    for kw, match in ((dict(colour=1.5), 'colour'), (dict(colour=-0.1), 'colour'), (dict(colour=float('nan')), 'colour'),
                      (dict(colour=[0.1, 0.2, 0.3]), 'colour'), (dict(colour=[[0.1, 0.2]]), 'colour'), (dict(max_gain=0.5), 'max_gain'),
                      (dict(max_gain=float('inf')), 'max_gain'), (dict(max_gain=float('nan')), 'max_gain'), (dict(max_gain='big'), 'max_gain'),
                      (dict(colour=0.5, boxes=huge), r'boxes: row 0 has 6400000000 pixels'),
                      (dict(colour=[0.0, 0.5], donor_boxes=huge), r'donor_boxes: row 0 has 6400000000 pixels')):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            MP.plan_morph(**args)
    # without colour matching such a box is what it was: accepted
    assert MP.plan_morph(**dict(good, boxes=huge)).rows.tolist() == [list(r) for r in huge]
    assert MP.plan_morph(**dict(good, boxes=huge, colour=0.0, max_gain=4.0)).max_gain == 4.0
    # PhotoMorph: the fields, and their defaults for a caller of the earlier signature
    pm = MP.PhotoMorph(None, None, None, np.zeros((2, 5)), np.zeros((2, 5)), None, None, None, None, [0, 1], [1, 0], 0.0, 2)
    assert pm.colour.tolist() == [0.0, 0.0] and pm.colour_gain is None and pm.colour_flags is None and pm.max_gain is None
    pm = MP.PhotoMorph(None, None, None, np.zeros((2, 5)), np.zeros((2, 5)), None, None, None, None, [0, 1], [1, 0], 0.0, 2, [0.5, 1.0], 2.0,
                       'gain', 'flags')
    assert pm.colour.dtype == F32 and pm.colour.tolist() == [0.5, 1.0] and (pm.max_gain, pm.colour_gain, pm.colour_flags) == (2.0, 'gain', 'flags')


# ----------------------------------------------------------------------------------------------------------------------------
# the region
# ----------------------------------------------------------------------------------------------------------------------------
def test_integer_ellipse_against_a_float64_ellipse():
    """The restatement's integer test against the formula in float64 at every pixel of boxes 1 x 1, 1 x 7, 2 x 2 and 17 x 23 (and a few
    more): the two may disagree only where the float64 sum lies within rounding of 1, and there the integers decide.  Found: 0
    disagreements on all of them (no pixel centre of these boxes lies within 1e-12 of its ellipse)."""
    total = 0
    for H, W in ((1, 1), (1, 7), (2, 2), (17, 23), (64, 64), (5, 40), (10, 10), (3, 4)):
        got = CO.region((0, 0, 0, H, W), 1, [(H, W)])
        want, margin = CO.ellipse_f64(H, W)
        differ = got != want
        total += int(differ.sum())
        assert (np.abs(margin[differ]) <= 1e-12).all(), (H, W)
        # exact rational arithmetic on every pixel: Python integers do not round
        for i in range(H):
            for j in range(W):
                a, b = 2 * i + 1 - H, 2 * j + 1 - W
                assert bool(got[i, j]) == (a * a * W * W + b * b * H * H <= H * H * W * W), (H, W, i, j)
        assert got.sum() > 0 and (got.sum() == H * W) == (min(H, W) <= 2), 'boxes one or two pixels thin lie wholly inside'
        assert np.array_equal(got, got[::-1]) and np.array_equal(got, got[:, ::-1]), 'symmetric'
        if H == W:
            assert np.array_equal(got, got.T)
    print('\nCOLOUR ELLIPSE: %d disagreements between the integer test and the float64 formula' % total)
    assert not CO.region((0, 0, 0, 17, 23), 1, [(17, 23)])[0, 0], 'the corners of a face box are background'
    # a box in a photo: shifted, clipped, and the rows with the empty region
    hw = [(37, 53)]
    full = CO.region((0, 0, 0, 17, 23), 1, [(17, 23)])
    assert np.array_equal(CO.region((0, 10, 20, 27, 43), 1, hw)[10:27, 20:43], full) and CO.region((0, 10, 20, 27, 43), 1, hw).sum() == full.sum()
    assert np.array_equal(CO.region((0, -6, 40, 11, 63), 1, hw)[0:11, 40:53], full[6:, :13])
    for row in ((-1, 0, 0, 5, 5), (1, 0, 0, 5, 5), (0, 5, 5, 5, 9), (0, 9, 5, 5, 9), (0, -40000, -40000, 40000, 40000)):
        assert CO.region(row, 1, hw) is None, row
    assert not CO.region((0, 100, 100, 120, 130), 1, hw).any()
    assert CO.region((0, 0, 0, 1 << 15, 1 << 15), 1, hw) is not None, 'H W == 2^30 is served'
    ph = CO.stats_photos()
    s = CO.stats(ph, CO.stats_rows(65))
    assert s.dtype == np.uint64 and s[0].tolist() == [int(v) for v in ph[0][5, 9]] + [int(v) ** 2 for v in ph[0][5, 9]] + [1]
    assert s[:16, 6].tolist() == [1, 7, 4, 311, 3228, 160, 29, 0, 0, 0, 0, 0, 0, 0, 4420, 0] and not s[7:14].any() and (s[16:, 6] > 0).sum() > 40


# ----------------------------------------------------------------------------------------------------------------------------
# the gain rule: hand-derived known answers
# ----------------------------------------------------------------------------------------------------------------------------
def _sums(values):
    """uint64 [7] of a region given as a list of (r, g, b) pixels."""
    v = np.array(values, dtype=np.uint64).reshape(-1, 3)
    return np.concatenate([v.sum(axis=0), (v * v).sum(axis=0), [len(v)]]).astype(np.uint64)


def test_gain_rule_known_answers():
    one = np.ones(1, F32)
    # constant regions: g = 1 and o is the difference of the colours
    a, b = _sums([(200, 17, 99)] * 5), _sums([(90, 30, 99)] * 8)
    g, fl = CO.gain(a[None], b[None], one, 2.0)
    assert g.dtype == F32 and g.shape == (1, 3, 2) and fl.tolist() == [0]
    assert g[0].tolist() == [[1.0, 110.0], [1.0, -13.0], [1.0, 0.0]]
    # a donor with twice the face's spread: the face (10, 20) has mean 15, sd 5; the donor (100, 120) mean 110, sd 10: g = 0.5,
    # o = 15 - 0.5 * 110 = -40
    a, b = _sums([(10, 10, 10), (20, 20, 20)]), _sums([(100, 100, 100), (120, 120, 120)])
    g, fl = CO.gain(a[None], b[None], one, 2.0)
    assert g[0].tolist() == [[0.5, -40.0]] * 3 and fl.tolist() == [0]
    # ... taken half way: G = 1 + 0.5 * (0.5 - 1) = 0.75, O = 0.5 * -40 = -20
    assert CO.gain(a[None], b[None], [0.5], 2.0)[0][0].tolist() == [[0.75, -20.0]] * 3
    # the clamp at max_gain: the face's spread is 8 times the donor's (sd 40 against 5); g = 2, o = 60 - 2 * 15 = 30; with max_gain 8
    # the ratio itself, o = 60 - 8 * 15 = -60; the other way round g = 1 / 8 clamped to 1 / 2, o = 15 - 0.5 * 60 = -15
    a, b = _sums([(20, 20, 20), (100, 100, 100)]), _sums([(10, 10, 10), (20, 20, 20)])
    assert CO.gain(a[None], b[None], one, 2.0)[0][0].tolist() == [[2.0, 30.0]] * 3
    assert CO.gain(a[None], b[None], one, 8.0)[0][0].tolist() == [[8.0, -60.0]] * 3
    assert CO.gain(b[None], a[None], one, 2.0)[0][0].tolist() == [[0.5, -15.0]] * 3
    assert CO.gain(a[None], b[None], one, 1.0)[0][0].tolist() == [[1.0, 45.0]] * 3, 'max_gain 1: the means alone'
    # a flat donor under a face with spread: g = 1 by the rule (no division by zero), o = the difference of the means
    assert CO.gain(a[None], _sums([(7, 7, 7)] * 3)[None], one, 2.0)[0][0].tolist() == [[1.0, 53.0]] * 3
    # a zero count on either side: (1, 0) and the flag; a NaN or infinite amount likewise
    zero = np.zeros(7, np.uint64)
    for sa, sb, t in ((zero, b, 1.0), (a, zero, 1.0), (zero, zero, 0.5), (a, b, np.nan), (a, b, np.inf), (a, b, -np.inf)):
        g, fl = CO.gain(sa[None], sb[None], [t], 2.0)
        assert g[0].tolist() == [[1.0, 0.0]] * 3 and fl.tolist() == [1], t
    # amount 0: exactly (1, 0), whatever the regions
    rng = np.random.RandomState(3)
    sa = np.stack([_sums(rng.randint(0, 256, (rng.randint(1, 50), 3))) for _ in range(40)])
    sb = np.stack([_sums(rng.randint(0, 256, (rng.randint(1, 50), 3))) for _ in range(40)])
    g, fl = CO.gain(sa, sb, np.zeros(40, F32), 2.0)
    unit = np.tile(np.array([1.0, 0.0], F32), (40, 3, 1))
    assert np.array_equal(g, unit) and not fl.any(), 'as values: the offset 0 * o carries the sign of o, and x + -0 = x'
    # a donor region equal to the face's own: exactly (1, 0) for every amount
    g, fl = CO.gain(sa, sa, rng.uniform(0, 1, 40).astype(F32), 2.0)
    assert np.array_equal(g.view(np.uint32), unit.view(np.uint32)) and not fl.any()
    # in general the corrected donor has the face's mean and (inside the clamp) the face's spread
    g, fl = CO.gain(sa, sb, np.ones(40, F32), 1e6)
    _n, ma, sda = CO.moments(sa)
    _n, mb, sdb = CO.moments(sb)
    ok = sdb > 0
    assert np.allclose(g[..., 0] * mb + g[..., 1], ma, rtol=0, atol=1e-3 * (1 + np.abs(g[..., 0]) * 255))
    assert np.allclose((g[..., 0] * sdb)[ok], np.clip(sda[ok], sdb[ok] / 1e6, None), rtol=1e-6, atol=1e-6)
    # colour_moments, the host half of detector.colour_stats, is the same arithmetic (on int64 bits as the device tensor holds them)
    cnt, m, sd = MP.colour_moments(sa.view(np.int64))
    assert cnt.dtype == np.int64 and np.array_equal(cnt, sa[:, 6].astype(np.int64)) and np.array_equal(m, ma) and np.array_equal(sd, sda)
    cnt, m, sd = MP.colour_moments(np.zeros((1, 7), np.int64))
    assert cnt.tolist() == [0] and np.isnan(m).all() and np.isnan(sd).all()


# ----------------------------------------------------------------------------------------------------------------------------
# the f32 restatement of the morph with colour against the f64 one on the GPU test's case
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,m', R.KERNEL_SHAPES)
def test_f32_restatement_against_f64(K, m):
    """morph_reference's kernel case with gains from the rule at max_gain = 2 (amounts in [0.1, 1], one row at 0 and one at 1; gains
    0.55 .. 1.38, offsets up to 56 grey levels): morph_f32 against morph_f64, both driven by the f32-rounded coefficients and gains,
    differs by at most one grey level on fewer than 0.5 % of the covered pixels, morph's own cap.  Found on this case: 0 of 1825 covered
    pixels for every K, lam and feather but (K = 64, lam = 0, feather = 0.5), where 1 pixel differs by one level."""
    for lam in R.LAMS:
        case, poses, coef_a, coef_b, ctrl, flags, cond = R.fitted_case(K, m, lam)
        photos, rows, donors, drows, mu_a, mu_b, shape, texture = case
        gain, gflags, amount = CO.morph_gains(case)
        assert gflags.tolist() == [int(b in (R.BAD_DONOR_ROW, R.OUTSIDE_ROW) + tuple(R.BAD_IMAGE_ROWS)) for b in range(len(rows))]
        assert np.array_equal(gain[CO.AMOUNT_ZERO_ROW], np.tile(np.array([1.0, 0.0], F32), (3, 1))) and amount[CO.AMOUNT_ONE_ROW] == 1.0
        live = gain[gflags == 0]
        assert (live[..., 0] >= 0.5).all() and (live[..., 0] <= 2.0).all() and np.abs(live[..., 1]).max() > 10
        ca, cb = coef_a.astype(F32), coef_b.astype(F32)
        for feather in R.FEATHERS:
            ramp = WR.inv_ramp(rows, feather)
            ref64, covered = CO.morph_f64(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp, gain)
            ref32, cov32 = CO.morph_f32(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp, gain)
            n_diff, worst, _near, n_cov = UR.within_cap(ref32, ref64, covered, WR.no_band(photos))
            print('\nCOLOUR MORPH f32 vs f64 K=%d anchors=%d lam=%g feather=%g: %d of %d covered pixels differ (max %d)' % (
                K, m, lam, feather, n_diff, n_cov, worst))
            assert all(np.array_equal(x, y) for x, y in zip(covered, cov32)) and n_cov > 1500
            # the gain changes the picture, and gain (1, 0) is the morph without colour in both restatements
            plain32, _c = R.morph_f32(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp)
            assert sum(int((a != b).any(axis=2).sum()) for a, b in zip(ref32, plain32)) > 0.3 * n_cov
            if lam == 0.0:
                unit = np.tile(np.array([1.0, 0.0], F32), (len(rows), 3, 1))
                same32, _c = CO.morph_f32(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp, unit)
                same64, _c = CO.morph_f64(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp, unit)
                plain64, _c = R.morph_f64(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp)
                assert all(np.array_equal(a, b) for a, b in zip(same32, plain32)) and all(np.array_equal(a, b) for a, b in zip(same64, plain64))


def test_flat_photos_swap_returns_the_photo():
    """Two flat photos of different colours, shape = 0, texture = 1, colour = 1: the corrected donor IS the face's colour, so the photo
    returns bit for bit from both restatements (and without colour matching the donor's colour arrives)."""
    photo, donor = CO.flat_photo(48, 56, (200, 17, 99)), CO.flat_photo(30, 20, (90, 30, 140))
    rows, drows = np.array([(0, 4, 20, 36, 52)], dtype=np.int32), np.array([(0, 3, 2, 25, 18)], dtype=np.int32)
    rng = np.random.RandomState(3)
    mu_a, mu_b = R.landmarks(6, 1, rng)
    coef_a, coef_b, ctrl, flags, _cond = R.fit2_f64(mu_a, mu_b, R.blend_f32(mu_a, mu_b, [0.0]), 2, 0.0)
    gain, gflags = CO.gain(CO.stats([photo], rows), CO.stats([donor], drows), [1.0], 2.0)
    assert gain[0].tolist() == [[1.0, 110.0], [1.0, -13.0], [1.0, -41.0]] and not gflags.any()
    for feather in R.FEATHERS:
        ramp = WR.inv_ramp(rows, feather)
        for fn in (CO.morph_f64, CO.morph_f32):
            out, cov = fn([photo], rows, [donor], drows, ctrl, coef_a, coef_b, [1.0], ramp, gain)
            assert np.array_equal(out[0], photo) and cov[0].sum() == 32 * 32
        out, _c = R.morph_f32([photo], rows, [donor], drows, ctrl, coef_a, coef_b, [1.0], ramp)
        assert feather > 0 or (out[0][4:36, 20:52] == (90, 30, 140)).all()
