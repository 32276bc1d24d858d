"""The seamless morph on the MI355X: imm_seam_fit's ring and flags bit for bit against the restatement (tests/seam_reference.py) and its
differences against the f32 and f64 restatements, imm_morph_seam_u8 within morph's cap of the f32 and f64 restatements with and without a
gain, the header's consequences (a) to (d), one block per row and the grid-stride loop, guarded buffers with a wild ring, wild differences
and wild shares, and LandmarkDetector.morph(mask='hull', seamless=...) with the script."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compose_reference as CR                                               # noqa: E402
import guarded                                                               # noqa: E402
import hull_reference as HR                                                  # noqa: E402
import morph_reference as R                                                  # noqa: E402
import seam_reference as SR                                                  # noqa: E402
import unalign_reference as UR                                               # noqa: E402
import warp_reference as WR                                                  # noqa: E402
from alignment_reference import smooth_photo                                  # noqa: E402
from dataset_fixtures import make_celeba_tree                                 # noqa: E402
from test_colour_gpu import _count_calls                                      # noqa: E402
from test_detector_gpu import _run_script, _write_config                      # noqa: E402
from test_generator_gpu import make_model as make_generator_model             # noqa: E402
from test_hull_gpu import run_hull_fit, run_hull_morph                        # noqa: E402
from test_morph_gpu import DONOR_BOXES, DONOR_SIZES, device_fit, packed_mask, run_morph, same_values      # noqa: E402
from test_unalign_gpu import SURFACE_BOXES, SURFACE_SIZES                     # noqa: E402
from test_warp_gpu import dev                                                 # noqa: E402

from imm_amd.inference import plan_buckets                                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 128
F32, F64 = np.float32, np.float64


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def run_seam_fit(ops, photos, rows, donors, drows, poses, grow, edges, hflags, B, ctrl, coef_a, coef_b, texture, gain=None, garbage=0x5A):
    """imm_seam_fit in guarded buffers, the outputs prefilled with garbage -> (ring f32 [n, B, 2], diff f32 [n, B, 3], flags int32 [n]) as
    host arrays."""
    n = len(rows)
    buf, offs, hw = CR.pack(photos)
    dbuf, doffs, dhw = CR.pack(donors)
    guarded.reset()
    ring, diff, flags = guarded.out((n, B, 2), torch.float32, DEV), guarded.out((n, B, 3), torch.float32, DEV), guarded.out((n,), torch.int32, DEV)
    for t in (ring, diff, flags):
        t.view(torch.uint8).fill_(garbage)
    g = lambda a, dt: guarded.inp(_t(np.asarray(a, dt)), DEV)
    ops.seam_fit(g(poses, F32), g(rows, np.int32), g(grow, F32), g(edges, F32), g(hflags, np.int32), g(SR.dirs(B), F64), g(buf, np.uint8),
                 dev(ops, offs), dev(ops, hw), g(dbuf, np.uint8), dev(ops, doffs), dev(ops, dhw), g(drows, np.int32), g(texture, F32),
                 g(ctrl, F32), g(coef_a, F32), g(coef_b, F32), None if gain is None else g(gain, F32), ring, diff, flags)
    torch.cuda.synchronize()
    guarded.check_guards()
    return ring.cpu().numpy(), diff.cpu().numpy(), flags.cpu().numpy()


def run_seam_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, edges, soft, ring, diff, seamless, gain=None,
                   launches=None, links=None, max_pixels=None):
    """test_morph_gpu.run_morph for imm_morph_seam_u8: ring f32 [n, B, 2], diff f32 [n, B, 3] and seamless f32 [n] as well."""
    return run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, launches, links, max_pixels=max_pixels,
                     gain=gain, edges=edges, soft=soft, ring=ring, diff=diff, seamless=seamless)


def case_gains(n):
    """test_seam_cpu's gains: 0.8 .. 1.2 and offsets -20 .. 20."""
    return np.stack([np.linspace(0.8, 1.2, 3 * n).reshape(n, 3), np.linspace(-20, 20, 3 * n).reshape(n, 3)], axis=2).astype(F32)


_DEVICE_CASES = {}


def device_case(ops, K, m):
    """seam_reference.kernel_case with the device's fit and the device's lines (checked against the restatement bit for bit), computed
    once per shape and shared: (case, poses, coef_a, coef_b, ctrl, edges, hull flags)."""
    if (K, m) not in _DEVICE_CASES:
        case = SR.kernel_case(K, m)
        photos, rows, donors, drows, mu_a, mu_b, shape, texture, grow, seamless = case
        poses, coef_a, coef_b, ctrl, _flags = device_fit(ops, mu_a, mu_b, shape, m, 0.0)
        assert same_values(poses, R.blend_f32(mu_a, mu_b, shape))
        edges, hflags = run_hull_fit(ops, poses, rows, grow)
        want, wflags = HR.hull_fit(poses, rows, grow)
        assert same_values(edges, want) and np.array_equal(hflags, wflags)
        _DEVICE_CASES[(K, m)] = (case, poses, coef_a, coef_b, ctrl, edges, hflags)
    return _DEVICE_CASES[(K, m)]


def diff_bound(M, photos, donors):
    """How far two evaluations of one difference may lie apart when both follow the rule and differ only in rounding and in their log:
    each of the two places is a sum of M + 3 products and a handful of scalings, every one rounded at a magnitude of at most the
    largest photo side P, so a place moves by at most (M + 8) * 2^-24 * P pixels per evaluation; a bilinear sample of u8 pixels changes
    by at most 255 per pixel along each axis, and own - mix holds two such samples at full weight, on both axes, in both evaluations."""
    P = max(max(p.shape[:2]) for p in list(photos) + list(donors))
    return 2 * 2 * 2 * 255.0 * (M + 8) * 2.0 ** -24 * P


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the seam fit
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', SR.RINGS)
@pytest.mark.parametrize('K,m', SR.KERNEL_SHAPES)
def test_seam_fit_kernel(ops, K, m, B):
    """seam_reference.kernel_case (overlapping rows, a hull that leaves its box, a centroid outside its box, a flagged hull, a row that is
    not active): the ring bit for bit against ring_f64 rounded to f32 and the flags equal; the differences against diff_f32 and
    diff_f64 at the device's own ring within diff_bound (the library logf is inside, and the f64 form has another order of
    operations); flagged rows and the row that is not active get 0.  With and without a gain, output buffers guarded and prefilled
    with garbage; the rows one by one give the bits of the launch of all."""
    case, poses, coef_a, coef_b, ctrl, edges, hflags = device_case(ops, K, m)
    photos, rows, donors, drows, mu_a, mu_b, shape, texture, grow, seamless = case
    n, M = len(rows), ctrl.shape[1]
    want, wflags = SR.ring_f64(poses, rows, edges, hflags, SR.dirs(B))
    bound = diff_bound(M, photos, donors)
    for gain in (None, case_gains(n)):
        ring, diff, flags = run_seam_fit(ops, photos, rows, donors, drows, poses, grow, edges, hflags, B, ctrl, coef_a, coef_b, texture, gain)
        assert np.array_equal(flags, wflags), (flags, wflags)
        assert same_values(ring, want), 'the ring differs from the restatement in its bits'
        d32 = SR.diff_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ring, flags, gain)
        d64 = SR.diff_f64(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ring, flags, gain)
        e32, e64 = float(np.abs(diff - d32).max()), float(np.abs(diff.astype(F64) - d64).max())
        print('\nSEAM FIT K=%d M=%d B=%d gain=%s: max |diff - f32| %.3g, max |diff - f64| %.3g (bound %.3g), max |diff| %.1f' % (
            K, M, B, gain is not None, e32, e64, bound, float(np.abs(diff).max())))
        assert np.isfinite(diff).all() and e32 <= bound and e64 <= bound
        assert not diff[flags != 0].any() and not diff[SR.INACTIVE_ROW].any() and np.abs(diff).max() > 20
        assert flags[SR.OUTSIDE_ROW] & 1 and flags[SR.NAN_ROW] & 1 and not flags[[0, 1, SR.SIDES_ROW, SR.INACTIVE_ROW, n - 1]].any()
    again = run_seam_fit(ops, photos, rows, donors, drows, poses, grow, edges, hflags, B, ctrl, coef_a, coef_b, texture, gain, garbage=0xFF)
    assert same_values(again[0], ring) and same_values(again[1], diff) and np.array_equal(again[2], flags)
    for b in (0, SR.SIDES_ROW, SR.OUTSIDE_ROW, SR.NAN_ROW):                     # a grid of one workgroup
        pick = [b]
        one = run_seam_fit(ops, photos, rows[pick], donors, drows[pick], poses[pick], grow[pick], edges[pick], hflags[pick], B, ctrl[pick],
                           coef_a[pick], coef_b[pick], texture[pick], gain[pick])
        assert same_values(one[0], ring[pick]) and same_values(one[1], diff[pick]) and np.array_equal(one[2], flags[pick]), b


def test_seam_fit_of_a_square_by_hand(ops):
    """The flat case's square (tests/test_seam_cpu.py): the samples along the axes and on the corners, exactly, and the integer
    difference of the two flat colours at every sample."""
    photo, donor, rows, drows, poses = SR.flat_case()
    one = np.ones(1, F32)
    edges, hflags = run_hull_fit(ops, poses, rows, one)
    _p, coef_a, coef_b, ctrl, fflags = device_fit(ops, poses, poses, np.zeros(1, F32), 2, 0.0)
    assert not fflags.any() and not coef_a.any() and not coef_b.any()
    ring, diff, flags = run_seam_fit(ops, [photo], rows, [donor], drows, poses, one, edges, hflags, 16, ctrl, coef_a, coef_b, one)
    assert flags.tolist() == [0]
    assert ring[0, [0, 4, 8, 12]].tolist() == [[27.5, 16.0], [16.0, 27.5], [4.5, 16.0], [16.0, 4.5]]
    assert ring[0, [2, 6, 10, 14]].tolist() == [[27.5, 27.5], [4.5, 27.5], [4.5, 4.5], [27.5, 4.5]]
    assert (diff == np.array((110, -13, -41), F32)).all()


# ----------------------------------------------------------------------------------------------------------------------------
# 2. the morph with the membrane against the restatements
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('feather', SR.FEATHERS)
@pytest.mark.parametrize('K,m', SR.KERNEL_SHAPES)
def test_morph_seam_kernel_parity(ops, K, m, feather):
    """imm_morph_seam_u8 on seam_reference.kernel_case at rings of 16 and 128 samples, with and without a gain, against the f32 and the
    f64 restatement driven by the kernel's own coefficients, lines, ring and differences: at most one grey level on at most 0.5 % of
    the pixels with w > 0 (unalign_reference.within_cap); every other byte of the packed buffer is the input's.  On this case the two
    restatements ALONE differ on 0 of 1 867 (K = 3), 0 of 4 867 (K = 10) and 0 to 3 of 5 731 (K = 64) such pixels
    (tests/test_seam_cpu.py)."""
    case, poses, coef_a, coef_b, ctrl, edges, hflags = device_case(ops, K, m)
    photos, rows, donors, drows, mu_a, mu_b, shape, texture, grow, seamless = case
    n = len(rows)
    soft, ramp = HR.inv_soft(rows, SR.MASK_FEATHER), WR.inv_ramp(rows, feather)
    for B in SR.RINGS:
        for gain in (None, case_gains(n)):
            ring, diff, flags = run_seam_fit(ops, photos, rows, donors, drows, poses, grow, edges, hflags, B, ctrl, coef_a, coef_b, texture, gain)
            got, buf = run_seam_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, edges, soft, ring, diff,
                                      seamless, gain)
            ref32, cov32 = SR.morph_seam_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ramp, edges, soft, ring, diff, seamless, gain)
            ref64, covered = SR.morph_seam_f64(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ramp, edges, soft, ring, diff, seamless, gain)
            out = CR.unpack(got, photos)
            n32 = sum(int((a != b).any(axis=2).sum()) for a, b in zip(out, ref32))
            n64 = sum(int((a != b).any(axis=2).sum()) for a, b in zip(out, ref64))
            n_cov = sum(int(c.sum()) for c in covered)
            print('\nSEAM MORPH KERNEL K=%d anchors=%d ring=%d feather=%g gain=%s: %d of %d pixels with w > 0 differ from the f32 restatement, '
                  '%d from the f64 one' % (K, m, B, feather, gain is not None, n32, n_cov, n64))
            assert all(np.array_equal(x, y) for x, y in zip(covered, cov32))
            UR.within_cap(out, ref32, covered, WR.no_band(photos))
            UR.within_cap(out, ref64, covered, WR.no_band(photos))
            inside = packed_mask(covered)
            assert inside.sum() == 3 * n_cov and np.array_equal(got[~inside], buf[~inside])
            hull, _buf = run_hull_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, edges, soft, gain)
            assert (got != hull).sum() > 0.3 * n_cov, 'the membrane is at work'


# ----------------------------------------------------------------------------------------------------------------------------
# 3. the consequences, byte for byte
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,m', [(10, 2), (64, 4)])
def test_seamless_zero_and_flagged_rows_are_the_hull_morph(ops, K, m):
    """(a) every seamless = 0: mix + 0 * r, the bytes of imm_morph_hull_u8 on the whole canvas, with and without a gain.  (b) the row
    whose centroid lies outside its box, flagged by imm_seam_fit, at seamless = 1: the bytes of the hull morph, alone in a launch and
    among the others."""
    case, poses, coef_a, coef_b, ctrl, edges, hflags = device_case(ops, K, m)
    photos, rows, donors, drows, mu_a, mu_b, shape, texture, grow, seamless = case
    n = len(rows)
    soft = HR.inv_soft(rows, SR.MASK_FEATHER)
    for B, gain, feather in ((128, None, 0.0), (16, case_gains(n), 0.125)):
        ring, diff, flags = run_seam_fit(ops, photos, rows, donors, drows, poses, grow, edges, hflags, B, ctrl, coef_a, coef_b, texture, gain)
        hull, buf = run_hull_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, edges, soft, gain)
        zero, _buf = run_seam_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, edges, soft, ring, diff,
                                    np.zeros(n, F32), gain)
        assert np.array_equal(zero, hull) and not np.array_equal(hull, buf), (B, 'seamless = 0')
        only = np.zeros(n, F32)
        only[SR.OUTSIDE_ROW] = 1.0
        assert flags[SR.OUTSIDE_ROW] and not diff[SR.OUTSIDE_ROW].any()
        got, _buf = run_seam_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, edges, soft, ring, diff, only, gain)
        assert np.array_equal(got, hull), (B, 'a flagged row among the others')
        pick = [SR.OUTSIDE_ROW]
        args = (photos, rows[pick], donors, drows[pick], ctrl[pick], coef_a[pick], coef_b[pick], texture[pick], feather, edges[pick], soft[pick])
        alone, buf1 = run_seam_morph(ops, *args, ring[pick], diff[pick], only[pick], None if gain is None else gain[pick])
        hull1, _buf = run_hull_morph(ops, *args, None if gain is None else gain[pick])
        assert np.array_equal(alone, hull1) and not np.array_equal(hull1, buf1), (B, 'a flagged row alone')


@pytest.mark.parametrize('B', SR.RINGS)
def test_flat_photos_come_back_bit_for_bit(ops, B):
    """(c) two flat photos of different colours, swapped (shape = 0, texture = 1) at seamless = 1, with and without a gain, at feather 0
    and 0.125: the photo comes back bit for bit; the same call at seamless = 0 changes all 529 pixels of the mask."""
    photo, donor, rows, drows, poses = SR.flat_case()
    one = np.ones(1, F32)
    edges, hflags = run_hull_fit(ops, poses, rows, one)
    _p, coef_a, coef_b, ctrl, fflags = device_fit(ops, poses, poses, np.zeros(1, F32), 2, 0.0)
    assert not fflags.any() and not hflags.any() and not coef_a.any() and not coef_b.any()
    soft = HR.inv_soft(rows, 0.1)
    for gain, step in ((None, (110, -13, -41)), (np.tile(np.array([1.0, 7.0], F32), (1, 3, 1)), (103, -20, -48))):
        ring, diff, flags = run_seam_fit(ops, [photo], rows, [donor], drows, poses, one, edges, hflags, B, ctrl, coef_a, coef_b, one, gain)
        assert not flags.any() and (diff == np.array(step, F32)).all(), 'every diff is the same integer triple'
        for feather in SR.FEATHERS:
            args = (ops, [photo], rows, [donor], drows, ctrl, coef_a, coef_b, one, feather, edges, soft, ring, diff)
            got, buf = run_seam_morph(*args, one, gain)
            assert np.array_equal(got, buf), (B, feather, 'the photo, bit for bit')
            plain, _buf = run_seam_morph(*args, 0 * one, gain)
            assert (CR.unpack(plain, [photo])[0] != photo).any(axis=2).sum() == 23 * 23, 'at seamless = 0 the donor is pasted'


def wild_seam(ring, diff, seamless, seed=8):
    """NaN, +-inf, 1e30 and random values in ring, diff and seamless: inputs the entry point accepts and the rule defines."""
    rng = np.random.RandomState(seed)
    r, d, s = ring.copy(), diff.copy(), seamless.copy()
    r[0, ::3, 0], r[1, 1::2] = np.nan, rng.uniform(-100, 100, r[1, 1::2].shape)
    r[2, 5:9], r[6, :, 1] = (np.inf, -np.inf), F32(1e30)
    d[0, 1::4], d[1, :, 1], d[2] = F32(1e30), np.nan, rng.uniform(-1e6, 1e6, d[2].shape)
    d[6, ::2, 2] = -np.inf
    s[0], s[1], s[2], s[6] = 1e30, np.nan, np.inf, -5.0
    return r, d, s


def test_morph_seam_split_invariance_and_addresses(ops):
    """(d) the rows as one launch, as two, and one by one give the same bytes; so does ONE block of 256 threads per row (max_box_pixels =
    1) and three or four blocks per row (max_box_pixels = 700, far below the boxes of 1 920 and more pixels: the grid-stride loop).  A
    row met on a link walk takes ITS ring, ITS differences and ITS share: swapping the two overlapping rows' changes the bytes.  Then
    NaN, inf, 1e30 and random values in ring, diff and seamless, with random links: every guard band holds, bytes change only inside
    the boxes, the launches still agree, and with the links in order the bytes are the f32 restatement's."""
    K, m, B = 10, 2, 128
    case, poses, coef_a, coef_b, ctrl, edges, hflags = device_case(ops, K, m)
    photos, rows, donors, drows, mu_a, mu_b, shape, texture, grow, seamless = case
    n = len(rows)
    soft = HR.inv_soft(rows, SR.MASK_FEATHER)
    gains = case_gains(n)
    ring, diff, flags = run_seam_fit(ops, photos, rows, donors, drows, poses, grow, edges, hflags, B, ctrl, coef_a, coef_b, texture)
    boxes = packed_mask(CR.box_mask(photos, rows))
    rng = np.random.RandomState(9)
    links = rng.randint(-5, n + 5, size=(n, 2)).astype(np.int32)
    for (rg, df, sm), gain, feather in (((ring, diff, seamless), None, 0.0), ((ring, diff, seamless), gains, 0.125),
                                        (wild_seam(ring, diff, seamless), None, 0.125)):
        args = (ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, edges, soft, rg, df, sm, gain)
        one, buf = run_seam_morph(*args)
        two, _ = run_seam_morph(*args, launches=[list(range(0, 1)), list(range(1, n))])
        each, _ = run_seam_morph(*args, launches=[[i] for i in range(n)])
        assert np.array_equal(one, two) and np.array_equal(one, each), feather
        assert np.array_equal(run_seam_morph(*args, max_pixels=1)[0], one), 'one block per row'
        assert np.array_equal(run_seam_morph(*args, max_pixels=700)[0], one), 'the grid-stride loop'
        assert not np.array_equal(one, buf) and np.array_equal(one[~boxes], buf[~boxes])
        ref32, covered = SR.morph_seam_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, WR.inv_ramp(rows, feather), edges, soft,
                                           rg, df, sm, gain)
        UR.within_cap(CR.unpack(one, photos), ref32, covered, WR.no_band(photos))
        inside = packed_mask(covered)
        assert np.array_equal(one[~inside], buf[~inside])
        wild, _ = run_seam_morph(*args, links=links)
        assert np.array_equal(wild[~boxes], buf[~boxes]), 'random links: nothing outside the boxes is written'
    i, j = 0, 1                                                                 # the two overlapping rows of photo 0
    sw_ring, sw_diff, sw_s = ring.copy(), diff.copy(), seamless.copy()
    sw_ring[[i, j]], sw_diff[[i, j]], sw_s[[i, j]] = ring[[j, i]], diff[[j, i]], seamless[[j, i]]
    a, _ = run_seam_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, 0.0, edges, soft, ring, diff, seamless)
    b, _ = run_seam_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, 0.0, edges, soft, sw_ring, sw_diff, sw_s)
    assert not np.array_equal(a, b)
    ref, cov = SR.morph_seam_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, WR.inv_ramp(rows, 0.0), edges, soft, sw_ring,
                                 sw_diff, sw_s)
    UR.within_cap(CR.unpack(b, photos), ref, cov, WR.no_band(photos))


# ----------------------------------------------------------------------------------------------------------------------------
# 4. LandmarkDetector.morph(mask='hull', seamless=...)
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def m128(ops):
    return make_generator_model(10, S, 4)


@pytest.fixture(scope='module')
def scene():
    """test_morph_gpu's scene: seven rows over six photos, two buckets at max_batch = 4, landmarks on a jittered grid for both sides."""
    ims = [smooth_photo(h, w, 60 + i) for i, (h, w) in enumerate(SURFACE_SIZES)]
    dons = [smooth_photo(h, w, 80 + i) for i, (h, w) in enumerate(DONOR_SIZES)]
    lm_a, lm_b = R.landmarks(10, len(SURFACE_BOXES), np.random.RandomState(12))
    return ims, dons, lm_a, lm_b


def test_detector_morph_seamless_zero_is_the_hull_morph(ops, m128, scene):
    cfg, model, eng, P, St = m128
    ims, dons, lm_a, lm_b = scene
    det = model.landmark_detector(S, max_batch=4)
    n = len(SURFACE_BOXES)
    kw = dict(boxes=SURFACE_BOXES, donor_boxes=DONOR_BOXES, shape=np.linspace(0.0, 1.0, n).astype(F32), texture=0.8, landmarks=lm_a,
              donor_landmarks=lm_b, mask='hull')
    det.morph(ims, dons, **kw)                                                                 # (captures and allocations out of the way)
    for colour in (0.0, 1.0):
        (plain, pm0), calls0 = _count_calls(ops, lambda: det.morph(ims, dons, colour=colour, return_transform=True, **kw))
        (zero, pmz), callsz = _count_calls(ops, lambda: det.morph(ims, dons, colour=colour, seamless=0.0, ring=16, return_transform=True, **kw))
        assert calls0 == callsz and calls0.count('imm_morph_hull_u8') == 2 and not [c for c in calls0 if 'seam' in c], 'launch for launch'
        assert all(torch.equal(x, y) for x, y in zip(plain, zero)), 'byte for byte'
        for pm in (pm0, pmz):
            assert pm.seamless is None and pm.ring is None and pm.seam_ring is None and pm.seam_diff is None and pm.seam_flags is None
        # with the membrane: one imm_seam_fit per bucket in front of the paste, imm_morph_seam_u8 in place of imm_morph_hull_u8
        (out, pm), calls = _count_calls(ops, lambda: det.morph(ims, dons, colour=colour, seamless=1.0, ring=16, return_transform=True, **kw))
        assert calls.count('imm_seam_fit') == 2 and calls.count('imm_morph_seam_u8') == 2 and 'imm_morph_hull_u8' not in calls
        assert [c for c in calls if c != 'imm_seam_fit'] == [c.replace('imm_morph_hull_u8', 'imm_morph_seam_u8') for c in calls0]
        assert all(calls[i + 1] == 'imm_morph_seam_u8' for i, c in enumerate(calls) if c == 'imm_seam_fit')
        assert not all(torch.equal(x, y) for x, y in zip(plain, out))
        assert pm.ring == 16 and tuple(pm.seam_ring.shape) == (n, 16, 2) and tuple(pm.seam_diff.shape) == (n, 16, 3) and pm.seam_ring.is_cuda
        assert pm.seam_flags.dtype == torch.int32 and torch.equal(pm.flags, pm0.flags) and torch.equal(pm.hull_flags, pm0.hull_flags)
    with pytest.raises(ValueError, match="needs mask='hull'"):
        det.morph(ims, dons, boxes=SURFACE_BOXES, donor_boxes=DONOR_BOXES, seamless=0.5)
    for bad, match in ((dict(seamless=1.5), 'seamless'), (dict(ring=8), 'ring'), (dict(seamless=[0.5] * 3), 'seamless'), (dict(ring=64.0), 'ring')):
        with pytest.raises(ValueError, match=match):
            det.morph(ims, dons, boxes=SURFACE_BOXES, donor_boxes=DONOR_BOXES, mask='hull', **bad)


def test_detector_morph_seamless_against_the_restatement(ops, m128, scene):
    from imm_amd import keypoints as KP
    cfg, model, eng, P, St = m128
    ims, dons, lm_a, lm_b = scene
    det = model.landmark_detector(S, max_batch=4)
    n = len(SURFACE_BOXES)
    assert len(plan_buckets(n, 4)) == 2
    rows, drows = KP.check_boxes(SURFACE_BOXES, len(ims)), KP.check_boxes(DONOR_BOXES, len(dons))
    shape = np.linspace(0.0, 1.0, n).astype(F32)
    texture = np.array([1.0, 0.3, 0.5, 1.0, 0.8, 0.6, 0.2], dtype=F32)
    for colour, seamless, B, feather, m in ((0.0, 1.0, 128, 0.125, 2), (1.0, np.linspace(0.0, 1.0, n).astype(F32), 16, 0.0, 0)):
        out, pm = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=shape, texture=texture, feather=feather, anchors=m,
                            landmarks=lm_a, donor_landmarks=lm_b, return_transform=True, colour=colour, mask='hull', seamless=seamless, ring=B)
        torch.cuda.synchronize()
        s = np.broadcast_to(np.asarray(seamless, F32), (n,))
        assert np.array_equal(pm.seamless, s) and pm.ring == B and not pm.flags.any() and not pm.hull_flags.any()
        poses, edges, hflags = pm.poses.cpu().numpy(), pm.hull_edges.cpu().numpy(), pm.hull_flags.cpu().numpy()
        ring, diff, flags = pm.seam_ring.cpu().numpy(), pm.seam_diff.cpu().numpy(), pm.seam_flags.cpu().numpy()
        want, wflags = SR.ring_f64(poses, rows, edges, hflags, SR.dirs(B))
        assert ring.dtype == F32 and same_values(ring, want) and np.array_equal(flags, wflags) and not flags.any(), 'PhotoMorph.seam_ring, bit for bit'
        coef_a, coef_b, ctrl = pm.coef_a.cpu().numpy(), pm.coef_b.cpu().numpy(), pm.ctrl.cpu().numpy()
        gain = pm.colour_gain.cpu().numpy() if colour else None
        d64 = SR.diff_f64(ims, rows, dons, drows, ctrl, coef_a, coef_b, texture, ring, flags, gain)
        assert np.abs(diff.astype(F64) - d64).max() <= diff_bound(ctrl.shape[1], ims, dons)
        for i in (0, n - 1):
            f = pm.seam_field(i)
            H, W = int(rows[i, 3] - rows[i, 1]), int(rows[i, 4] - rows[i, 2])
            rr, cc = np.divmod(np.arange(H * W), W)
            assert f.dtype == F32 and f.shape == (H, W, 3) and np.array_equal(f.reshape(-1, 3), SR.field(ring[i], diff[i], rr, cc, F32))
        ref64, covered = SR.morph_seam_f64(ims, rows, dons, drows, ctrl, coef_a, coef_b, texture, WR.inv_ramp(rows, feather), edges, pm.inv_soft,
                                           ring, diff, s, gain)
        got = [o.cpu().numpy() for o in out]
        n_diff, worst, _near, n_cov = UR.within_cap(got, ref64, covered, WR.no_band(ims))
        hull = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=shape, texture=texture, feather=feather, anchors=m, landmarks=lm_a,
                         donor_landmarks=lm_b, colour=colour, mask='hull')
        moved = sum(int((x != p.cpu().numpy()).any(axis=2).sum()) for x, p in zip(got, hull))
        print('\nMORPH(seamless) colour=%g ring=%d feather=%g anchors=%d: %d of %d pixels with w > 0 differ from the f64 restatement (max %d); '
              '%d differ from seamless=0' % (colour, B, feather, m, n_diff, n_cov, worst, moved))
        assert moved > 0.1 * n_cov and all(np.array_equal(x[~c], im[~c]) for x, im, c in zip(got, ims, covered))
        # a second call gives the same bytes and leaves the first call's result alone
        before = [o.clone() for o in out]
        again = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=shape, texture=texture, feather=feather, anchors=m, landmarks=lm_a,
                          donor_landmarks=lm_b, colour=colour, mask='hull', seamless=seamless, ring=B)
        assert all(torch.equal(x, y) for x, y in zip(before, again)) and all(torch.equal(x, y) for x, y in zip(before, out))
    assert all(np.array_equal(im, smooth_photo(h, w, 60 + i)) for i, (im, (h, w)) in enumerate(zip(ims, SURFACE_SIZES)))


def test_generate_script_morphs_seamlessly(ops, m128, tmp_path, capsys):
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
    rows = [(names[0], 20, 10, 180, 150), (names[2], -10, 30, 120, 170)]
    boxes = str(tmp_path / 'faces.csv')
    with open(boxes, 'w') as f:
        f.write('file,y0,x0,y1,x1\n' + ''.join('%s,%d,%d,%d,%d\n' % r for r in rows))
    donor_dir = tmp_path / 'donors'
    donor_dir.mkdir()
    donor = (smooth_photo(120, 100, 3) * 0.5 + 20).astype(np.uint8)
    Image.fromarray(donor).save(str(donor_dir / 'a.png'))
    script = os.path.join(ROOT, 'scripts', 'generate.py')
    base = ['--configs', conf, '--checkpoint', ckpt, '--appearance-dir', imdir, '--boxes', boxes, '--batch-size', '4']
    swap = base + ['--morph', '--donor-dir', str(donor_dir), '--shape', '0', '--texture', '1', '--feather', '0.0']
    common = swap + ['--mask', 'hull', '--grow', '4']
    det = LandmarkDetector.from_checkpoint(load_configs([conf]).model, ckpt, image_size=S, max_batch=4, device=DEV)
    photos = [pixels[n] for n in names]
    api_rows = [(names.index(r[0]),) + r[1:] for r in rows]
    kw = dict(shape=0.0, texture=1.0, feather=0.0, mask='hull', grow=4.0)
    hull = det.morph(photos, [donor], api_rows, None, **kw)
    out_dir = str(tmp_path / 'out')
    _run_script(script, common + ['--seamless', '0.75', '--ring', '32', '--out-dir', out_dir])
    assert '2 faces morphed in 4 photos, 1 step ->' in capsys.readouterr().out
    want = det.morph(photos, [donor], api_rows, None, seamless=0.75, ring=32, **kw)
    for n, w in zip(names, want):
        png = np.asarray(Image.open(os.path.join(out_dir, n.replace('.jpg', '.png'))))
        assert np.array_equal(png, w.cpu().numpy()), n
    assert not all(torch.equal(w, p) for w, p in zip(want, hull)), 'the flag changes the picture'
    for extra, match in ((['--seamless', '2'], 'seamless'), (['--seamless', '1', '--ring', '8'], 'ring')):
        with pytest.raises(ValueError, match=match):
            _run_script(script, common + extra + ['--out-dir', str(tmp_path / 'no')])
    with pytest.raises(ValueError, match="needs mask='hull'"):
        _run_script(script, swap + ['--seamless', '1', '--out-dir', str(tmp_path / 'no')])
    with pytest.raises(ValueError, match='go with --morph'):
        _run_script(script, base + ['--seamless', '1', '--out-dir', str(tmp_path / 'no')])
