"""Colour matching on the MI355X: imm_colour_stats_u8 against numpy as integers, imm_colour_gain bit for bit against the restatement
(tests/colour_reference.py), imm_morph_colour_u8 within morph's cap of the f32 restatement, the identities byte for byte, invariance
under splitting a call into launches, guarded buffers with wild gains, and LandmarkDetector.morph(colour=...) / colour_stats with the
script."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colour_reference as CO                                                # noqa: E402
import compose_reference as CR                                               # noqa: E402
import guarded                                                               # noqa: E402
import morph_reference as R                                                  # noqa: E402
import unalign_reference as UR                                               # noqa: E402
import warp_reference as WR                                                  # noqa: E402
from alignment_reference import smooth_photo                                  # noqa: E402
from dataset_fixtures import make_celeba_tree                                 # noqa: E402
from test_detector_gpu import _run_script, _write_config                      # noqa: E402
from test_generator_gpu import make_model as make_generator_model             # noqa: E402
from test_morph_gpu import DONOR_BOXES, DONOR_SIZES, box_area, device_fit, packed_mask, run_morph      # noqa: E402
from test_unalign_gpu import SURFACE_BOXES, SURFACE_SIZES                     # noqa: E402
from test_warp_gpu import dev                                                 # noqa: E402

from imm_amd import morphing as MP                                            # noqa: E402
from imm_amd.inference import plan_buckets                                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 128
F32 = np.float32
UNIT = np.array([1.0, 0.0], F32)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def run_stats(ops, photos, rows, max_pixels=None, garbage=0x5A):
    """imm_colour_stats_u8 over the packed photos; the buffer and sums in guarded buffers, sums prefilled with garbage -> uint64 [n, 7]."""
    buf, offs, hw = CR.pack(photos)
    guarded.reset()
    src = guarded.inp(_t(buf), DEV)
    sums = guarded.out((len(rows), 7), torch.int64, DEV)
    sums.view(torch.uint8).fill_(garbage)
    ops.colour_stats_u8(src, dev(ops, offs), dev(ops, hw), dev(ops, rows), box_area(rows) if max_pixels is None else max_pixels, sums)
    torch.cuda.synchronize()
    guarded.check_guards()
    assert np.array_equal(src.cpu().numpy(), buf), 'the buffer is read only'
    return sums.cpu().numpy().view(np.uint64)


def run_gain(ops, sums_a, sums_b, amount, max_gain):
    """imm_colour_gain in guarded buffers -> (gain f32 [n, 3, 2], flags int32 [n]) as host arrays."""
    n = len(sums_a)
    guarded.reset()
    gain, flags = guarded.out((n, 3, 2), torch.float32, DEV), guarded.out((n,), torch.int32, DEV)
    ops.colour_gain(guarded.inp(_t(np.asarray(sums_a).view(np.int64)), DEV), guarded.inp(_t(np.asarray(sums_b).view(np.int64)), DEV),
                    guarded.inp(_t(np.asarray(amount, F32)), DEV), max_gain, gain, flags)
    torch.cuda.synchronize()
    guarded.check_guards()
    return gain.cpu().numpy(), flags.cpu().numpy()


def run_colour_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, gain, launches=None, links=None,
                     donor_is_src=False, max_pixels=None):
    """test_morph_gpu.run_morph for imm_morph_colour_u8: gain f32 [n, 3, 2] in a guarded buffer as well."""
    return run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, launches, links, donor_is_src, max_pixels,
                     gain=gain)


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the statistics, exact
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 65])
def test_colour_stats_kernel(ops, n):
    """Photos 37 x 53, 64 x 70 and 9 x 11 (odd widths); boxes 1 x 1, 1 x 7, 2 x 2, 17 x 23, 64 x 64, over the photo's edges, wholly
    outside, empty, image index -1 and n_images, H W > 2^30 (colour_reference.STATS_ROWS), then random ones."""
    photos, rows = CO.stats_photos(), CO.stats_rows(n)
    want = CO.stats(photos, rows)
    got = run_stats(ops, photos, rows)
    assert got.dtype == np.uint64 and np.array_equal(got, want), 'sums differ from numpy as integers'
    # max_box_pixels understated: ONE block of 256 walks every box through the grid-stride loop; other garbage in front
    assert np.array_equal(run_stats(ops, photos, rows, max_pixels=1, garbage=0xFF), want)
    if n == 65:
        assert want[4, 6] > 2 * 256 and not want[7:14].any() and not want[15].any() and (want[:, 6] > 0).sum() > 40
        # the rows one by one (a grid of one row) and a buffer of one photo
        for b in (3, 4, 5, 8, 13, 15):
            assert np.array_equal(run_stats(ops, photos, rows[b:b + 1]), want[b:b + 1]), b
    one = np.array([(0, 0, 0, 9, 11)], dtype=np.int32)
    assert np.array_equal(run_stats(ops, photos[2:], one), CO.stats(photos[2:], one))


# ----------------------------------------------------------------------------------------------------------------------------
# 2. the gain, bit for bit
# ----------------------------------------------------------------------------------------------------------------------------
def test_colour_gain_kernel(ops):
    photos, rows = CO.stats_photos(), CO.stats_rows(65)
    sums = run_stats(ops, photos, rows)
    rng = np.random.RandomState(21)
    a, b = sums.copy(), sums[rng.permutation(len(sums))].copy()
    flat = lambda c, k: np.array([c * k] * 3 + [c * c * k] * 3 + [k], dtype=np.uint64)
    a[3], b[4], a[5], b[5] = flat(77, 40), flat(200, 9), flat(10, 5), flat(250, 7)           # a flat region on each side, and on both
    b[6] = a[6]                                                                               # the donor region is the face's own
    amount = rng.uniform(0, 1, len(a)).astype(F32)
    both = [i for i in np.nonzero((a[:, 6] > 0) & (b[:, 6] > 0))[0] if i > 6]              # rows with pixels on both sides
    i_nan, i_inf, i_zero, i_one, i_ninf = both[:5]
    amount[i_nan], amount[i_inf], amount[i_zero], amount[i_one], amount[i_ninf] = np.nan, np.inf, 0.0, 1.0, -np.inf
    zero_a, zero_b = np.nonzero(a[:, 6] == 0)[0], np.nonzero(b[:, 6] == 0)[0]
    assert len(zero_a) >= 8 and len(zero_b) >= 8 and a[3, 6] and b[3, 6] and a[4, 6] and b[4, 6] and a[6, 6]
    for max_gain in (2.0, 1.0, 8.0):
        got, flags = run_gain(ops, a, b, amount, max_gain)
        want, wflags = CO.gain(a, b, amount, max_gain)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), 'gain differs from the restatement in its bits (max_gain %g)' % max_gain
        assert np.array_equal(flags, wflags) and flags[i_nan] == flags[i_inf] == flags[i_ninf] == 1 and flags[i_zero] == flags[i_one] == 0
        assert flags[zero_a].all() and flags[zero_b].all() and np.array_equal(got[flags == 1], np.tile(UNIT, (int(flags.sum()), 3, 1)))
        assert np.array_equal(got[i_zero], np.tile(UNIT, (3, 1))), 'amount 0 gives (1, 0)'
        assert np.array_equal(got[6].view(np.uint32), np.tile(UNIT, (3, 1)).view(np.uint32)), 'x / x = 1 and m - 1 * m = 0'
        assert (got[[3, 4, 5], :, 0] != 1).sum() <= 6 and np.isfinite(got).all()
        live = flags == 0
        assert (got[live, :, 0] >= 1 - amount[live, None] * (1 - 1 / max_gain) - 1e-6).all()
        assert (got[live, :, 0] <= 1 + amount[live, None] * (max_gain - 1) + 1e-6).all()
    assert len(np.unique(got[live, :, 0])) > 20, 'the gains are not all at the clamp'
    # one row
    got, flags = run_gain(ops, a[:1], b[40:41], [0.5], 2.0)
    want, wflags = CO.gain(a[:1], b[40:41], [0.5], 2.0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(flags, wflags)


# ----------------------------------------------------------------------------------------------------------------------------
# 3. the morph with colour against the f32 restatement
# ----------------------------------------------------------------------------------------------------------------------------
def device_gains(ops, case):
    """The gains of morph_reference.kernel_case's rows from the two kernels, checked against the restatement bit for bit."""
    photos, rows, donors, drows = case[:4]
    want, wflags, amount = CO.morph_gains(case)
    sa, sb = run_stats(ops, photos, rows), run_stats(ops, donors, drows)
    assert np.array_equal(sa, CO.stats(photos, rows)) and np.array_equal(sb, CO.stats(donors, drows))
    gain, flags = run_gain(ops, sa, sb, amount, CO.MAX_GAIN)
    assert np.array_equal(gain.view(np.uint32), want.view(np.uint32)) and np.array_equal(flags, wflags)
    return gain


@pytest.mark.parametrize('feather', R.FEATHERS)
@pytest.mark.parametrize('K,m', R.KERNEL_SHAPES)
def test_morph_colour_kernel_parity(ops, K, m, feather):
    """imm_morph_colour_u8 against colour_reference.morph_f32 driven by the kernel's own coefficients and gains (the rule at max_gain =
    2): at most one grey level, on fewer than 0.5 % of the covered pixels (morph's own cap, a condition).  The photos and poses are
    morph's kernel case, on which the f32 and f64 restatements ALONE differ on 0 of 1825 covered pixels, and on 1 at K = 64, lam = 0,
    feather = 0.5 (tests/test_colour_cpu.py::test_f32_restatement_against_f64)."""
    case = R.kernel_case(K, m)
    photos, rows, donors, drows, mu_a, mu_b, shape, texture = case
    gain = device_gains(ops, case)
    for lam in R.LAMS:
        _poses, coef_a, coef_b, ctrl, flags = device_fit(ops, mu_a, mu_b, shape, m, lam)
        assert flags.tolist() == [int(b == R.NAN_ROW) for b in range(len(rows))]
        got, buf = run_colour_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, gain)
        ramp = WR.inv_ramp(rows, feather)
        ref32, covered = CO.morph_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ramp, gain)
        ref64, _cov = CO.morph_f64(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ramp, gain)
        out = CR.unpack(got, photos)
        d32 = [np.abs(a.astype(int) - b.astype(int)).max(axis=2) for a, b in zip(out, ref32)]
        n64 = sum(int((a != b).any(axis=2).sum()) for a, b in zip(out, ref64))
        n_cov = sum(int(c.sum()) for c in covered)
        print('\nCOLOUR MORPH KERNEL K=%d anchors=%d lam=%g feather=%g: %d of %d covered pixels differ from the f32 restatement (max %d), %d '
              'from the f64 one' % (K, m, lam, feather, sum(int((d > 0).sum()) for d in d32), n_cov, max(int(d.max()) for d in d32), n64))
        UR.within_cap(out, ref32, covered, WR.no_band(photos))
        # every byte no row writes is the input's
        inside = packed_mask(covered)
        assert inside.sum() == 3 * n_cov and np.array_equal(got[~inside], buf[~inside])
        # and the gain is at work: the bytes are not those of imm_morph_u8
        plain, _buf = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather)
        assert (got != plain).sum() > 0.3 * n_cov
    silent = sorted(R.SILENT_ROWS)
    for pick in [[b] for b in silent] + [silent]:
        got, buf = run_colour_morph(ops, photos, rows[pick], donors, drows[pick], ctrl[pick], coef_a[pick], coef_b[pick], texture[pick], feather,
                                    gain[pick])
        assert np.array_equal(got, buf), pick


# ----------------------------------------------------------------------------------------------------------------------------
# 4. the identities, byte for byte on the whole canvas
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,m', [(10, 2), (64, 4)])
def test_morph_colour_identities(ops, K, m):
    photos, rows, donors, drows, mu_a, mu_b, shape, texture = R.kernel_case(K, m)
    n = len(rows)
    feathers = R.FEATHERS + (0.25,)
    # gain (1, 0) is imm_morph_u8
    _poses, coef_a, coef_b, ctrl, _flags = device_fit(ops, mu_a, mu_b, shape, m, 0.0)
    unit = np.tile(UNIT, (n, 3, 1))
    signed = unit.copy()
    signed[::2, :, 1] = -0.0                                                    # amount 0 leaves a zero of either sign
    for feather in feathers:
        plain, buf = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather)
        for g in (unit, signed):
            got, _buf = run_colour_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, g)
            assert np.array_equal(got, plain), feather
        assert not np.array_equal(plain, buf)
    # the donor is the face itself (same buffer, photo and box): the rule gives (1, 0) for every colour, and every byte returns
    own_rows = rows.copy()
    own_rows[list(R.BAD_IMAGE_ROWS), 0] = 0
    _poses, coef_a, coef_b, ctrl, _flags = device_fit(ops, mu_a, mu_a, shape, m, 0.0)
    sa = run_stats(ops, photos, rows)
    for colour in (0.0, 0.4, 1.0):
        gain, gflags = run_gain(ops, sa, sa, np.full(n, colour, F32), 2.0)
        assert np.array_equal(gain.view(np.uint32), unit.view(np.uint32)), 'a donor region equal to the face\'s own gives exactly (1, 0)'
        for tex in (0.0, 0.37, 1.0):
            for feather in feathers:
                got, buf = run_colour_morph(ops, photos, rows, photos, own_rows, ctrl, coef_a, coef_b, np.full(n, tex, F32), feather, gain,
                                            donor_is_src=True)
                assert np.array_equal(got, buf), (colour, tex, feather)


def test_flat_photos_swap_returns_the_photo(ops):
    """Two flat photos of different colours with shape = 0, texture = 1, colour = 1: the corrected donor IS the face's colour, so the
    photo returns bit for bit; without the gain the donor's colour arrives."""
    photos = [CO.flat_photo(48, 57, (200, 17, 99)), CO.flat_photo(21, 33, (5, 250, 128))]
    donors = [CO.flat_photo(30, 21, (90, 30, 140)), CO.flat_photo(40, 40, (255, 0, 64))]
    rows = np.array([(0, 4, 20, 36, 52), (1, -3, 5, 18, 40), (0, 10, 0, 45, 30)], dtype=np.int32)
    drows = np.array([(0, 3, 2, 25, 18), (1, 0, 0, 40, 40), (1, 5, -4, 30, 20)], dtype=np.int32)
    n = len(rows)
    mu_a, mu_b = R.landmarks(10, n, np.random.RandomState(8))
    _poses, coef_a, coef_b, ctrl, flags = device_fit(ops, mu_a, mu_b, np.zeros(n, F32), 2, 0.0)
    assert not flags.any() and not coef_a.any() and coef_b.any()
    gain, gflags = run_gain(ops, run_stats(ops, photos, rows), run_stats(ops, donors, drows), np.ones(n, F32), 2.0)
    assert gain[0].tolist() == [[1.0, 110.0], [1.0, -13.0], [1.0, -41.0]] and gain[1].tolist() == [[1.0, -250.0], [1.0, 250.0], [1.0, 64.0]]
    assert not gflags.any()
    one = np.ones(n, F32)
    for feather in R.FEATHERS:
        got, buf = run_colour_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, one, feather, gain)
        assert np.array_equal(got, buf), feather
        plain, _buf = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, one, feather)
        assert (plain != buf).sum() > 3000


# ----------------------------------------------------------------------------------------------------------------------------
# 5. split invariance, one block per row and addressing, with wild gains
# ----------------------------------------------------------------------------------------------------------------------------
def wild_gains(n, seed=4):
    rng = np.random.RandomState(seed)
    g = np.stack([rng.uniform(-3, 3, (n, 3)), rng.uniform(-300, 300, (n, 3))], axis=2).astype(F32)
    g[1::5, :, 0] = F32(1e30)
    g[2::5, 1, 1] = -np.inf
    g[3::5, 0, 0] = np.nan
    g[4::5, 2, 1] = np.inf
    return g


def test_morph_colour_split_invariance(ops):
    photos, rows, donors, drows, mu_a, mu_b, shape, texture = R.kernel_case(10, 2)
    _poses, coef_a, coef_b, ctrl, _flags = device_fit(ops, mu_a, mu_b, shape, 2, 0.0)
    n = len(rows)
    full = drows.copy()
    full[R.BAD_DONOR_ROW, 0] = 1                                              # all three mutually overlapping rows are live
    for gain in (device_gains(ops, R.kernel_case(10, 2)), wild_gains(n)):
        for feather, dr in ((0.0, drows), (0.125, drows), (0.125, full)):
            one, buf = run_colour_morph(ops, photos, rows, donors, dr, ctrl, coef_a, coef_b, texture, feather, gain)
            two, _ = run_colour_morph(ops, photos, rows, donors, dr, ctrl, coef_a, coef_b, texture, feather, gain,
                                      [list(range(0, 4)), list(range(4, n))])
            each, _ = run_colour_morph(ops, photos, rows, donors, dr, ctrl, coef_a, coef_b, texture, feather, gain, [[i] for i in range(n)])
            assert np.array_equal(one, two) and np.array_equal(one, each), feather
            # ONE block of 256 threads per row gives the same bytes
            assert np.array_equal(run_colour_morph(ops, photos, rows, donors, dr, ctrl, coef_a, coef_b, texture, feather, gain, max_pixels=1)[0], one)
            assert not np.array_equal(one, buf)
    # a row met on a link walk takes ITS gain, not the block's: swapping two overlapping rows' gains changes the bytes
    gain = device_gains(ops, R.kernel_case(10, 2))
    i, j = WR.OVERLAPPING[0], WR.OVERLAPPING[2]
    swapped = gain.copy()
    swapped[[i, j]] = gain[[j, i]]
    a, _ = run_colour_morph(ops, photos, rows, donors, full, ctrl, coef_a, coef_b, texture, 0.0, gain)
    b, _ = run_colour_morph(ops, photos, rows, donors, full, ctrl, coef_a, coef_b, texture, 0.0, swapped)
    assert not np.array_equal(a, b)
    ref, _cov = CO.morph_f32(photos, rows, donors, full, ctrl, coef_a, coef_b, texture, WR.inv_ramp(rows, 0.0), swapped)
    UR.within_cap(CR.unpack(b, photos), ref, _cov, WR.no_band(photos))


def test_morph_colour_addresses_nothing_outside_the_photos(ops):
    photos, rows, donors, drows, mu_a, mu_b, shape, texture = R.kernel_case(10, 2)
    _poses, coef_a, coef_b, ctrl, _flags = device_fit(ops, mu_a, mu_b, shape, 2, 0.0)
    rng = np.random.RandomState(9)
    n = len(rows)

    def wild(coef):
        w = coef.copy()
        w[1::4] *= F32(1e6)
        w[2::4] *= F32(1e30)
        w[3::4, 5] = np.inf
        w[0, 2, 1] = np.nan
        return w
    links = rng.randint(-5, n + 5, size=(n, 2)).astype(np.int32)
    far = drows.copy()
    far[0::3, 1:] += np.array([100000, -70000, 100000, -70000], dtype=np.int32)
    far[1, 1:] = (-(1 << 23), -(1 << 23), 1 << 23, 1 << 23)
    boxes = packed_mask(CR.box_mask(photos, rows[[b for b in range(n) if 0 <= rows[b, 0] < len(photos)]]))
    gains = wild_gains(n)
    for ca, cb in ((wild(coef_a), coef_b), (coef_a, wild(coef_b)), (wild(coef_a), wild(coef_b)), (coef_a, coef_b)):
        for lk in (None, links):
            for dr in (drows, far):
                got, buf = run_colour_morph(ops, photos, rows, donors, dr, ctrl, ca, cb, texture, 0.125, gains, links=lk)   # checks every guard band
                assert np.array_equal(got[~boxes], buf[~boxes])
    # wild gains, good everything else: the rows still write, and what they write is the restatement's (a NaN mix clamps to 0)
    got, buf = run_colour_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, 0.125, gains)
    ref32, covered = CO.morph_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, WR.inv_ramp(rows, 0.125), gains)
    UR.within_cap(CR.unpack(got, photos), ref32, covered, WR.no_band(photos))
    # the statistics with box rows that hold anything: every guard band stays, whatever the sums are
    junk = rng.randint(-2 ** 31, 2 ** 31 - 1, size=(64, 5), dtype=np.int64).astype(np.int32)
    junk[::2, 0] = rng.randint(0, len(photos), 32)
    junk[::4, 1:] = rng.randint(-50, 90, size=(16, 4))
    assert np.array_equal(run_stats(ops, photos, junk), CO.stats(photos, junk))
    assert np.array_equal(run_stats(ops, photos, junk, max_pixels=1), CO.stats(photos, junk))


# ----------------------------------------------------------------------------------------------------------------------------
# 6. LandmarkDetector.morph(colour=...) and colour_stats
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def m128(ops):
    return make_generator_model(10, S, 4)


@pytest.fixture(scope='module')
def scene():
    """test_morph_gpu's scene with the donor photos in other light: darker, flatter and tinted per channel."""
    ims = [smooth_photo(h, w, 60 + i) for i, (h, w) in enumerate(SURFACE_SIZES)]
    tint = np.array([0.55, 0.7, 0.4])
    dons = [np.clip(smooth_photo(h, w, 80 + i) * tint + (10, 25, 60), 0, 255).astype(np.uint8) for i, (h, w) in enumerate(DONOR_SIZES)]
    lm_a, lm_b = R.landmarks(10, len(SURFACE_BOXES), np.random.RandomState(12))
    return ims, dons, lm_a, lm_b


def _count_calls(ops, fn):
    """fn() with every library call of imm_amd.ops recorded by name."""
    names, call0 = [], ops.call
    ops.call = lambda name, *a: (names.append(name), call0(name, *a))[1]
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.call = call0
    return out, names


def test_detector_morph_colour_zero_is_the_morph(ops, m128, scene):
    cfg, model, eng, P, St = m128
    ims, dons, lm_a, lm_b = scene
    det = model.landmark_detector(S, max_batch=4)
    n = len(SURFACE_BOXES)
    kw = dict(boxes=SURFACE_BOXES, donor_boxes=DONOR_BOXES, shape=np.linspace(0.0, 1.0, n).astype(F32), texture=0.8, landmarks=lm_a,
              donor_landmarks=lm_b)
    det.morph(ims, dons, **kw)                                                                 # (captures and allocations out of the way)
    (plain, pm0), calls0 = _count_calls(ops, lambda: det.morph(ims, dons, return_transform=True, **kw))
    (zero, pmz), callsz = _count_calls(ops, lambda: det.morph(ims, dons, colour=0.0, max_gain=5.0, return_transform=True, **kw))
    (rows0, pmr), callsr = _count_calls(ops, lambda: det.morph(ims, dons, colour=[0.0] * n, return_transform=True, **kw))
    assert calls0 == callsz == callsr and calls0.count('imm_morph_u8') == 2 and not [c for c in calls0 if 'colour' in c]
    assert all(torch.equal(x, y) for x, y in zip(plain, zero)) and all(torch.equal(x, y) for x, y in zip(plain, rows0))
    assert pm0.colour_gain is None and pmz.colour_gain is None and pmz.colour_flags is None and pmz.colour.tolist() == [0.0] * n
    # with colour: two stats launches and one gain launch per call, in front of the buckets; the colour kernel per bucket
    (out, pm), calls = _count_calls(ops, lambda: det.morph(ims, dons, colour=1.0, return_transform=True, **kw))
    assert calls.count('imm_colour_stats_u8') == 2 and calls.count('imm_colour_gain') == 1 and calls.count('imm_morph_colour_u8') == 2
    assert 'imm_morph_u8' not in calls and len(calls) == len(calls0) + 3
    first = min(i for i, c in enumerate(calls) if c in ('imm_morph_poses', 'imm_warp_fit', 'imm_morph_colour_u8'))
    assert max(i for i, c in enumerate(calls) if c in ('imm_colour_stats_u8', 'imm_colour_gain')) < first
    assert not all(torch.equal(x, y) for x, y in zip(plain, out))


def test_detector_morph_colour_against_the_restatement(ops, m128, scene):
    from imm_amd import keypoints as KP
    cfg, model, eng, P, St = m128
    ims, dons, lm_a, lm_b = scene
    det = model.landmark_detector(S, max_batch=4)
    n = len(SURFACE_BOXES)
    assert len(plan_buckets(n, 4)) == 2
    rows, drows = KP.check_boxes(SURFACE_BOXES, len(ims)), KP.check_boxes(DONOR_BOXES, len(dons))
    shape = np.linspace(0.0, 1.0, n).astype(F32)
    texture = np.array([1.0, 0.3, 0.5, 1.0, 0.8, 0.6, 0.2], dtype=F32)
    sa, sb = CO.stats(ims, rows), CO.stats(dons, drows)
    for colour, max_gain, feather, m, lam in ((1.0, 2.0, 0.125, 2, 0.0), (np.linspace(1.0, 0.0, n).astype(F32), 1.25, 0.0, 0, 1e-2)):
        out, pm = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=shape, texture=texture, feather=feather, anchors=m, lam=lam,
                            landmarks=lm_a, donor_landmarks=lm_b, return_transform=True, colour=colour, max_gain=max_gain)
        torch.cuda.synchronize()
        amount = np.broadcast_to(np.asarray(colour, F32), (n,))
        want, wflags = CO.gain(sa, sb, amount, max_gain)
        gain = pm.colour_gain.cpu().numpy()
        assert gain.dtype == F32 and np.array_equal(gain.view(np.uint32), want.view(np.uint32)), 'PhotoMorph.colour_gain, bit for bit'
        assert np.array_equal(pm.colour_flags.cpu().numpy(), wflags) and not wflags.any()
        assert np.array_equal(pm.colour, amount) and pm.max_gain == max_gain and not pm.flags.any()
        assert np.abs(gain[..., 0] - 1).max() > 0.2 and np.abs(gain[..., 1]).max() > 10, 'the donors are lit unlike the photos'
        coef_a, coef_b, ctrl = pm.coef_a.cpu().numpy(), pm.coef_b.cpu().numpy(), pm.ctrl.cpu().numpy()
        ref64, covered = CO.morph_f64(ims, rows, dons, drows, ctrl, coef_a, coef_b, texture, WR.inv_ramp(rows, feather), gain)
        got = [o.cpu().numpy() for o in out]
        n_diff, worst, _near, n_cov = UR.within_cap(got, ref64, covered, WR.no_band(ims))
        plain = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=shape, texture=texture, feather=feather, anchors=m, lam=lam,
                          landmarks=lm_a, donor_landmarks=lm_b)
        moved = sum(int((g != p.cpu().numpy()).any(axis=2).sum()) for g, p in zip(got, plain))
        print('\nMORPH(colour) max_gain=%g feather=%g anchors=%d lam=%g: %d of %d covered pixels differ from the f64 restatement (max %d), %d '
              'differ from colour=0' % (max_gain, feather, m, lam, n_diff, n_cov, worst, moved))
        assert moved > 0.3 * n_cov and all(np.array_equal(g[~c], im[~c]) for g, im, c in zip(got, ims, covered))
        # a second call gives the same bytes and leaves the first call's result alone
        before = [o.clone() for o in out]
        again = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=shape, texture=texture, feather=feather, anchors=m, lam=lam,
                          landmarks=lm_a, donor_landmarks=lm_b, colour=colour, max_gain=max_gain)
        assert all(torch.equal(x, y) for x, y in zip(before, again)) and all(torch.equal(x, y) for x, y in zip(before, out))
    # the swap (shape 0, texture 1) at colour 1: over the face's ellipse the pasted donor has the face's mean but for what the spline
    # moves in or out of the donor's ellipse, a minority of its pixels: less than a quarter of the gap between the two photographs stays
    b = 3                                                                       # a box that no other row overlaps
    out = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=0.0, texture=1.0, feather=0.0, landmarks=lm_a, donor_landmarks=lm_b, colour=1.0,
                    max_gain=100.0)
    mask = CO.region(rows[b], len(ims), [im.shape[:2] for im in ims])
    mean_out, mean_in = out[rows[b, 0]].cpu().numpy()[mask].mean(axis=0), ims[rows[b, 0]][mask].mean(axis=0)
    mean_don = dons[drows[b, 0]][CO.region(drows[b], len(dons), [d.shape[:2] for d in dons])].mean(axis=0)
    assert np.abs(mean_out - mean_in).max() < 0.25 * np.abs(mean_don - mean_in).max(), (mean_out, mean_in, mean_don)
    # one donor row for all faces, colour per row, default max_gain
    one, pm1 = det.morph(ims, dons[:1], SURFACE_BOXES, [(0, 3, 5, 66, 80)], shape=0.25, landmarks=lm_a, donor_landmarks=lm_b[:1],
                         return_transform=True, colour=0.5)
    want, _f = CO.gain(sa, CO.stats(dons[:1], np.array([(0, 3, 5, 66, 80)] * n)), np.full(n, 0.5, F32), 2.0)
    assert np.array_equal(pm1.colour_gain.cpu().numpy().view(np.uint32), want.view(np.uint32)) and pm1.max_gain == 2.0
    for kw, match in ((dict(colour=1.5), 'colour'), (dict(colour=[0.5] * 3), 'colour'), (dict(colour=float('nan')), 'colour'),
                      (dict(max_gain=0.5), 'max_gain'), (dict(max_gain=float('inf')), 'max_gain'),
                      (dict(colour=0.5, boxes=[(0, -40000, -40000, 40000, 40000)] * n), '2\\^30')):
        args = dict(photos=ims, donors=dons, boxes=SURFACE_BOXES, donor_boxes=DONOR_BOXES)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            det.morph(**args)
    # the photos handed in are not written
    assert all(np.array_equal(im, smooth_photo(h, w, 60 + i)) for i, (im, (h, w)) in enumerate(zip(ims, SURFACE_SIZES)))


def test_detector_colour_stats(ops, m128, scene):
    cfg, model, eng, P, St = m128
    ims, dons, _a, _b = scene
    det = model.landmark_detector(S, max_batch=4)
    from imm_amd import keypoints as KP
    for photos, boxes in ((ims, SURFACE_BOXES), (dons, DONOR_BOXES), (ims, None), (CO.stats_photos(), CO.stats_rows(65)[[0, 1, 2, 3, 4, 5, 6, 7, 14]])):
        count, mean, sd = det.colour_stats(photos, boxes)
        rows = KP.check_boxes([(0, 0, a.shape[0], a.shape[1]) for a in photos] if boxes is None else boxes, len(photos))
        want = CO.stats(photos, rows)
        wn, wm, wsd = CO.moments(want)
        assert count.dtype == np.int64 and mean.dtype == np.float64 and sd.dtype == np.float64 and mean.shape == sd.shape == (len(rows), 3)
        assert np.array_equal(count, want[:, 6].astype(np.int64)) and np.array_equal(mean, wm, equal_nan=True) and np.array_equal(sd, wsd, equal_nan=True)
        # and plain numpy over the region's pixels
        for b, row in enumerate(rows.tolist()):
            mask = CO.region(row, len(photos), [p.shape[:2] for p in photos])
            if count[b]:
                px = photos[row[0]][mask].astype(np.float64)
                assert count[b] == len(px) and np.allclose(mean[b], px.mean(axis=0), rtol=1e-12) and np.allclose(sd[b], px.std(axis=0), atol=1e-6)
            else:
                assert not mask.any() and np.isnan(mean[b]).all()
    for kw, match in ((dict(photos=torch.zeros(2, 8, 8, 3)), 'u8 arrays'), (dict(photos=[]), 'u8 arrays'), (dict(boxes=[(9, 0, 0, 5, 5)]), 'names image'),
                      (dict(boxes=[(0, 5, 5, 5, 9)]), 'empty')):
        args = dict(photos=ims, boxes=None)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            det.colour_stats(**args)


def test_generate_script_morphs_with_colour(ops, m128, tmp_path, capsys):
    from PIL import Image
    from imm_amd.inference import LandmarkDetector
    from imm_amd.utils.config import load_configs
    cfg, model, eng, P, St = m128
    root = str(tmp_path / 'celeba')
    names, pixels = make_celeba_tree(root, n=4)
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, ckpt)
    conf = _write_config(tmp_path, root, str(tmp_path / 'logs'))
    imdir = os.path.join(root, 'Img', 'img_align_celeba_hq')
    rows = [(names[0], 20, 10, 180, 150), (names[2], -10, 30, 120, 170), (names[0], 100, 60, 215, 175)]
    boxes = str(tmp_path / 'faces.csv')
    with open(boxes, 'w') as f:
        f.write('file,y0,x0,y1,x1\n' + ''.join('%s,%d,%d,%d,%d\n' % r for r in rows))
    donor_dir = tmp_path / 'donors'
    donor_dir.mkdir()
    donor = (smooth_photo(120, 100, 3) * 0.5 + 20).astype(np.uint8)
    Image.fromarray(donor).save(str(donor_dir / 'a.png'))
    script = os.path.join(ROOT, 'scripts', 'generate.py')
    common = ['--configs', conf, '--checkpoint', ckpt, '--appearance-dir', imdir, '--boxes', boxes, '--batch-size', '4', '--morph',
              '--donor-dir', str(donor_dir), '--shape', '0.25', '--texture', '0.75', '--feather', '0.0']
    det = LandmarkDetector.from_checkpoint(load_configs([conf]).model, ckpt, image_size=S, max_batch=4, device=DEV)
    photos = [pixels[n] for n in names]
    api_rows = [(names.index(r[0]),) + r[1:] for r in rows]
    plain = det.morph(photos, [donor], api_rows, None, shape=0.25, texture=0.75, feather=0.0)
    for extra, kw in ((['--colour', '1'], dict(colour=1.0)), (['--colour', '0.5', '--max-gain', '1.5'], dict(colour=0.5, max_gain=1.5))):
        out_dir = str(tmp_path / ('out%d' % len(extra)))
        _run_script(script, common + extra + ['--out-dir', out_dir])
        assert '3 faces morphed in 4 photos, 1 step ->' in capsys.readouterr().out
        want = det.morph(photos, [donor], api_rows, None, shape=0.25, texture=0.75, feather=0.0, **kw)
        for n, w in zip(names, want):
            png = np.asarray(Image.open(os.path.join(out_dir, n.replace('.jpg', '.png'))))
            assert np.array_equal(png, w.cpu().numpy()), n
        assert not all(torch.equal(w, p) for w, p in zip(want, plain)), 'the flag changes the picture'
    for extra, match in ((['--colour', '2'], 'colour'), (['--colour', '1', '--max-gain', '0.5'], 'max_gain')):
        with pytest.raises(ValueError, match=match):
            _run_script(script, common + extra + ['--out-dir', str(tmp_path / 'no')])
    with pytest.raises(ValueError, match='go with --morph'):
        _run_script(script, [a for a in common if a != '--morph'][:10] + ['--colour', '1', '--out-dir', str(tmp_path / 'no')])
