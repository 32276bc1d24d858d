"""The landmark-hull mask of morph on the MI355X: imm_hull_fit bit for bit against the restatement (tests/hull_reference.py),
imm_morph_hull_u8 within morph's cap of the f32 and f64 restatements with and without a gain, the identities byte for byte, known
answers, invariance under splitting a call into launches, guarded buffers with wild lines, and LandmarkDetector.morph(mask='hull')
with the script."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colour_reference as CO                                                # noqa: E402
import compose_reference as CR                                               # noqa: E402
import guarded                                                               # noqa: E402
import hull_reference as HR                                                  # noqa: E402
import morph_reference as R                                                  # noqa: E402
import unalign_reference as UR                                               # noqa: E402
import warp_reference as WR                                                  # noqa: E402
from alignment_reference import smooth_photo                                  # noqa: E402
from dataset_fixtures import make_celeba_tree                                 # noqa: E402
from test_colour_gpu import _count_calls, run_colour_morph, wild_gains      # noqa: E402
from test_detector_gpu import _run_script, _write_config                      # noqa: E402
from test_generator_gpu import make_model as make_generator_model             # noqa: E402
from test_hull_cpu import flat_case                                           # noqa: E402
from test_morph_gpu import DONOR_BOXES, DONOR_SIZES, device_fit, packed_mask, run_morph, same_values      # noqa: E402
from test_unalign_gpu import SURFACE_BOXES, SURFACE_SIZES                     # noqa: E402

from imm_amd.inference import plan_buckets                                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 128
F32 = np.float32


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def run_hull_fit(ops, poses, rows, grow, garbage=0x5A):
    """imm_hull_fit in guarded buffers, the outputs prefilled with garbage -> (edges f32 [n, K, 3], flags int32 [n]) as host arrays."""
    n, K = poses.shape[:2]
    guarded.reset()
    edges, flags = guarded.out((n, K, 3), torch.float32, DEV), guarded.out((n,), torch.int32, DEV)
    edges.view(torch.uint8).fill_(garbage)
    flags.view(torch.uint8).fill_(garbage)
    ops.hull_fit(guarded.inp(_t(np.asarray(poses, F32)), DEV), guarded.inp(_t(np.asarray(rows, np.int32)), DEV),
                 guarded.inp(_t(np.asarray(grow, F32)), DEV), edges, flags)
    torch.cuda.synchronize()
    guarded.check_guards()
    return edges.cpu().numpy(), flags.cpu().numpy()


def run_hull_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, edges, soft, gain=None, launches=None,
                   links=None, max_pixels=None):
    """test_morph_gpu.run_morph for imm_morph_hull_u8: edges f32 [n, K, 3], soft f32 [n] and (unless None) gain f32 [n, 3, 2]."""
    return run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, launches, links, max_pixels=max_pixels,
                     gain=gain, edges=edges, soft=soft)


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the hull fit, bit for bit
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 3, 4, 10, 80])
@pytest.mark.parametrize('n', [1, 3, 65])
def test_hull_fit_kernel(ops, n, K):
    """hull_reference.fit_rows: the hand-made cases of the CPU test that have K points, random clouds in random boxes at grows 0.5, 1,
    1.25 and 1.5, then NaN and +-inf poses, NaN and infinite grows, an empty and an inverted box and boxes with sides of 100 000 and
    2^32 - 1; output buffers guarded and prefilled with garbage."""
    poses, rows, grow = HR.fit_rows(n, K)
    want, wflags = HR.hull_fit(poses, rows, grow)
    got, flags = run_hull_fit(ops, poses, rows, grow)
    assert np.array_equal(flags, wflags), (flags, wflags)
    assert same_values(got, want), 'edges differ from the restatement in their bits'
    got, flags = run_hull_fit(ops, poses, rows, grow, garbage=0xFF)
    assert same_values(got, want) and np.array_equal(flags, wflags)
    assert np.array_equal(got[flags != 0], np.tile(HR.NO_HULL, (int((flags != 0).sum()), K, 1)))
    if n == 65:
        assert (wflags & 1).sum() >= 6 and ((wflags == 0).sum() > 50) == (K >= 3)
        for b in (0, 1, 40, 64):                                               # the rows one by one: a grid of one workgroup
            one, f1 = run_hull_fit(ops, poses[b:b + 1], rows[b:b + 1], grow[b:b + 1])
            assert same_values(one, want[b:b + 1]) and np.array_equal(f1, wflags[b:b + 1]), b


def test_hull_fit_kernel_on_the_cases(ops):
    """Every hand-made case of the CPU test at grow 0.5, 1, 1.25 and 1.5, and the blended poses of morph's kernel case."""
    for name, points, hw, flag in HR.CASES:
        for g in (0.5, 1.0, 1.25, 1.5):
            poses, rows, grow = HR.case_inputs(points, hw, g)
            want, wflags = HR.hull_fit(poses, rows, grow)
            got, flags = run_hull_fit(ops, poses, rows, grow)
            assert same_values(got, want) and np.array_equal(flags, wflags) and flags.tolist() == [flag], (name, g)
    poses = np.array([[(-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5)]], F32)          # the unit square, by hand
    got, flags = run_hull_fit(ops, poses, np.array([(0, 7, 9, 23, 25)], np.int32), np.ones(1, F32))
    assert got[0].tolist() == [[0.0, 1.0, -4.0], [1.0, 0.0, -4.0], [0.0, -1.0, 12.0], [-1.0, 0.0, 12.0]] and flags.tolist() == [0]
    for K, m in R.KERNEL_SHAPES:
        case, poses = HR.kernel_poses(K, m)
        grow = np.full(len(poses), HR.GROW, F32)
        want, wflags = HR.hull_fit(poses, case[1], grow)
        got, flags = run_hull_fit(ops, poses, case[1], grow)
        assert same_values(got, want) and np.array_equal(flags, wflags), K


# ----------------------------------------------------------------------------------------------------------------------------
# 2. the morph with the mask against the restatements
# ----------------------------------------------------------------------------------------------------------------------------
def device_hull(ops, K, m, grow=HR.GROW):
    """morph's kernel case with the device's lines of its blended poses, checked against the restatement bit for bit."""
    case, poses = HR.kernel_poses(K, m)
    g = np.full(len(poses), grow, F32)
    edges, flags = run_hull_fit(ops, poses, case[1], g)
    want, wflags = HR.hull_fit(poses, case[1], g)
    assert same_values(edges, want) and np.array_equal(flags, wflags) and flags.tolist() == [3 * int(b == R.NAN_ROW) for b in range(len(g))]
    return case, edges


@pytest.mark.parametrize('feather', R.FEATHERS)
@pytest.mark.parametrize('K,m', R.KERNEL_SHAPES)
def test_morph_hull_kernel_parity(ops, K, m, feather):
    """imm_morph_hull_u8 on morph's kernel case at grow = 1.25, with and without colour_reference's gains, against the f32 and the f64
    restatement driven by the kernel's own coefficients and lines: at most one grey level on at most 0.5 % of the pixels with w > 0
    (unalign_reference.within_cap); every other byte of the packed buffer is the input's.  On this case the two restatements ALONE
    differ on 0 to 1 of 315 (K = 3), 883 (K = 10) and 1 502 (K = 64) such pixels (tests/test_hull_cpu.py)."""
    case, edges = device_hull(ops, K, m)
    photos, rows, donors, drows, mu_a, mu_b, shape, texture = case
    gains, _f, _a = CO.morph_gains(case)
    for lam, mf in zip(R.LAMS, HR.MASK_FEATHERS):
        _poses, coef_a, coef_b, ctrl, flags = device_fit(ops, mu_a, mu_b, shape, m, lam)
        soft, ramp = HR.inv_soft(rows, mf), WR.inv_ramp(rows, feather)
        plain, _buf = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather)
        for gain in (None, gains):
            got, buf = run_hull_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, edges, soft, gain)
            ref32, cov32 = HR.morph_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ramp, edges, soft, gain)
            ref64, covered = HR.morph_f64(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ramp, edges, soft, gain)
            out = CR.unpack(got, photos)
            n32 = sum(int((a != b).any(axis=2).sum()) for a, b in zip(out, ref32))
            n64 = sum(int((a != b).any(axis=2).sum()) for a, b in zip(out, ref64))
            n_cov = sum(int(c.sum()) for c in covered)
            print('\nHULL MORPH KERNEL K=%d anchors=%d lam=%g feather=%g mask_feather=%g gain=%s: %d of %d pixels with w > 0 differ from the '
                  'f32 restatement, %d from the f64 one' % (K, m, lam, feather, mf, gain is not None, n32, n_cov, n64))
            assert all(np.array_equal(x, y) for x, y in zip(covered, cov32))
            UR.within_cap(out, ref32, covered, WR.no_band(photos))
            UR.within_cap(out, ref64, covered, WR.no_band(photos))
            # every byte with w <= 0, every byte outside the boxes and the padding between the photos is the input's
            inside = packed_mask(covered)
            assert inside.sum() == 3 * n_cov and np.array_equal(got[~inside], buf[~inside])
            assert (got != buf).sum() > 0.3 * n_cov and (got != plain).sum() > 0.1 * n_cov, 'the mask is at work'
    # the silent rows write nothing, each alone in a launch and all of them together; nor does a row whose hull is flagged
    silent = sorted(R.SILENT_ROWS)
    for pick in [[b] for b in silent] + [silent]:
        got, buf = run_hull_morph(ops, photos, rows[pick], donors, drows[pick], ctrl[pick], coef_a[pick], coef_b[pick], texture[pick], feather,
                                  edges[pick], soft[pick], gains[pick])
        assert np.array_equal(got, buf), pick
    flagged = edges.copy()
    for b in (2, 4):
        flagged[b] = HR.NO_HULL
        got, buf = run_hull_morph(ops, photos, rows[[b]], donors, drows[[b]], ctrl[[b]], coef_a[[b]], coef_b[[b]], texture[[b]], feather,
                                  flagged[[b]], soft[[b]])
        assert np.array_equal(got, buf), b
    got, _buf = run_hull_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, flagged, soft)
    ref32, covered = HR.morph_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ramp, flagged, soft)
    UR.within_cap(CR.unpack(got, photos), ref32, covered, WR.no_band(photos))


def test_flat_photos_hard_edge_known_answer(ops):
    """Two flat photos of colours A and B, shape = 0, texture = 1, feather = 0 and a hard edge (inv_soft = 1e30): B exactly at the 312
    pixels strictly inside the polygon (counted in integers), A elsewhere.  No restatement is involved but for the lines' bits."""
    photo, donor, rows, drows, poses, inside = flat_case()
    edges, flags = run_hull_fit(ops, poses, rows, np.ones(1, F32))
    assert flags.tolist() == [0] and same_values(edges, HR.hull_fit(poses, rows, np.ones(1, F32))[0])
    _p, coef_a, coef_b, ctrl, fflags = device_fit(ops, poses, poses, np.zeros(1, F32), 2, 0.0)
    assert not fflags.any() and not coef_a.any() and not coef_b.any()
    want = photo.copy()
    want[4:36, 20:52][inside] = (90, 30, 140)
    got, buf = run_hull_morph(ops, [photo], rows, [donor], drows, ctrl, coef_a, coef_b, np.ones(1, F32), 0.0, edges, np.array([1e30], F32))
    assert inside.sum() == 312 and np.array_equal(CR.unpack(got, [photo])[0], want)
    gain = np.tile(np.array([1.0, 7.0], F32), (1, 3, 1))
    got, buf = run_hull_morph(ops, [photo], rows, [donor], drows, ctrl, coef_a, coef_b, np.ones(1, F32), 0.0, edges, np.array([1e30], F32), gain)
    want[4:36, 20:52][inside] = (97, 37, 147)
    assert np.array_equal(CR.unpack(got, [photo])[0], want)


# ----------------------------------------------------------------------------------------------------------------------------
# 3. byte for byte, no tolerance
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,m', [(10, 2), (64, 4)])
def test_morph_hull_identities(ops, K, m):
    """A hull that holds the whole box with w = 1 everywhere - the unit square about the frame's centre grown 16 times, whose edges lie
    3.5 box sides outside the box, with inv_soft = 1000 - gives paste_ramp * 1: the bytes of imm_morph_u8 on the whole canvas, with a
    gain those of imm_morph_colour_u8, and gain (1, 0) those of no gain."""
    photos, rows, donors, drows, mu_a, mu_b, shape, texture = case = R.kernel_case(K, m)
    n = len(rows)
    square = np.tile(np.array([[(-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5)]], F32), (n, 1, 1))
    edges, flags = run_hull_fit(ops, square, rows, np.full(n, 16.0, F32))
    assert not flags.any()
    soft = np.full(n, 1000.0, F32)
    _poses, coef_a, coef_b, ctrl, _flags = device_fit(ops, mu_a, mu_b, shape, m, 0.0)
    gains, _f, _a = CO.morph_gains(case)
    unit = np.tile(np.array([1.0, 0.0], F32), (n, 3, 1))
    for feather in R.FEATHERS + (0.25,):
        plain, buf = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather)
        got, _buf = run_hull_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, edges, soft)
        assert np.array_equal(got, plain) and not np.array_equal(plain, buf), feather
        got, _buf = run_hull_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, edges, soft, unit)
        assert np.array_equal(got, plain), feather
        coloured, _buf = run_colour_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, gains)
        got, _buf = run_hull_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, edges, soft, gains)
        assert np.array_equal(got, coloured) and not np.array_equal(coloured, plain), feather


# ----------------------------------------------------------------------------------------------------------------------------
# 4. split invariance, one block per row and addressing, with wild lines
# ----------------------------------------------------------------------------------------------------------------------------
def wild_edges(edges, seed=6):
    rng = np.random.RandomState(seed)
    e = edges.copy()
    n = len(e)
    e[1::5] = rng.uniform(-3, 3, e[1::5].shape)
    e[2::5, ::2, 0] = np.nan
    e[3::5, 1::2, 2] = np.inf
    e[3::5, 0, 1] = -np.inf
    e[4::5, :, :2] *= F32(1e30)
    soft = rng.uniform(0.05, 2.0, n).astype(F32)
    soft[0::4], soft[1::7], soft[2::7], soft[5::9] = 1e30, np.nan, np.inf, -1.0
    return e, soft


def test_morph_hull_split_invariance(ops):
    case, edges = device_hull(ops, 10, 2)
    photos, rows, donors, drows, mu_a, mu_b, shape, texture = case
    _poses, coef_a, coef_b, ctrl, _flags = device_fit(ops, mu_a, mu_b, shape, 2, 0.0)
    n = len(rows)
    full = drows.copy()
    full[R.BAD_DONOR_ROW, 0] = 1                                              # all three mutually overlapping rows are live
    gains, _f, _a = CO.morph_gains(case)
    for e, soft in ((edges, HR.inv_soft(rows, 0.1)), wild_edges(edges)):
        for feather, dr, gain in ((0.0, drows, None), (0.125, drows, gains), (0.125, full, None), (0.125, full, wild_gains(n))):
            one, buf = run_hull_morph(ops, photos, rows, donors, dr, ctrl, coef_a, coef_b, texture, feather, e, soft, gain)
            two, _ = run_hull_morph(ops, photos, rows, donors, dr, ctrl, coef_a, coef_b, texture, feather, e, soft, gain,
                                    [list(range(0, 4)), list(range(4, n))])
            each, _ = run_hull_morph(ops, photos, rows, donors, dr, ctrl, coef_a, coef_b, texture, feather, e, soft, gain, [[i] for i in range(n)])
            assert np.array_equal(one, two) and np.array_equal(one, each), feather
            # ONE block of 256 threads per row gives the same bytes
            assert np.array_equal(run_hull_morph(ops, photos, rows, donors, dr, ctrl, coef_a, coef_b, texture, feather, e, soft, gain,
                                                 max_pixels=1)[0], one)
            assert not np.array_equal(one, buf)
    # a row met on a link walk takes ITS lines and ITS inv_soft, not the block's: swapping two overlapping rows' changes the bytes, and
    # the result is the restatement's
    soft = HR.inv_soft(rows, 0.1)
    i, j = WR.OVERLAPPING[0], WR.OVERLAPPING[2]
    swapped, sw_soft = edges.copy(), soft.copy()
    swapped[[i, j]], sw_soft[[i, j]] = edges[[j, i]], F32(0.5) * soft[[j, i]]
    a, _ = run_hull_morph(ops, photos, rows, donors, full, ctrl, coef_a, coef_b, texture, 0.0, edges, soft)
    b, _ = run_hull_morph(ops, photos, rows, donors, full, ctrl, coef_a, coef_b, texture, 0.0, swapped, sw_soft)
    assert not np.array_equal(a, b)
    ref, cov = HR.morph_f32(photos, rows, donors, full, ctrl, coef_a, coef_b, texture, WR.inv_ramp(rows, 0.0), swapped, sw_soft)
    UR.within_cap(CR.unpack(b, photos), ref, cov, WR.no_band(photos))


def test_morph_hull_addresses_nothing_outside_the_photos(ops):
    """Wild lines (NaN, +-inf, 1e30, random) and a wild inv_soft (1e30, NaN, inf, negative) together with wild coefficients, wild gains,
    random links and far donor boxes: inputs the entry point accepts and the rule defines.  Every guard band holds, nothing outside
    the boxes is written, and with everything else in order the bytes are the restatement's."""
    case, edges = device_hull(ops, 10, 2)
    photos, rows, donors, drows, mu_a, mu_b, shape, texture = case
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
    e, soft = wild_edges(edges)
    gains = wild_gains(n)
    for ca, cb in ((wild(coef_a), coef_b), (coef_a, wild(coef_b)), (wild(coef_a), wild(coef_b)), (coef_a, coef_b)):
        for lk in (None, links):
            for dr, gain in ((drows, None), (far, gains)):
                got, buf = run_hull_morph(ops, photos, rows, donors, dr, ctrl, ca, cb, texture, 0.125, e, soft, gain, links=lk)
                assert np.array_equal(got[~boxes], buf[~boxes])
    for gain in (None, gains):
        got, buf = run_hull_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, 0.125, e, soft, gain)
        ref32, covered = HR.morph_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, WR.inv_ramp(rows, 0.125), e, soft, gain)
        UR.within_cap(CR.unpack(got, photos), ref32, covered, WR.no_band(photos))
        inside = packed_mask(covered)
        assert np.array_equal(got[~inside], buf[~inside]) and inside.any()


# ----------------------------------------------------------------------------------------------------------------------------
# 5. LandmarkDetector.morph(mask='hull')
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


def test_detector_morph_mask_none_is_the_morph(ops, m128, scene):
    cfg, model, eng, P, St = m128
    ims, dons, lm_a, lm_b = scene
    det = model.landmark_detector(S, max_batch=4)
    n = len(SURFACE_BOXES)
    kw = dict(boxes=SURFACE_BOXES, donor_boxes=DONOR_BOXES, shape=np.linspace(0.0, 1.0, n).astype(F32), texture=0.8, landmarks=lm_a,
              donor_landmarks=lm_b)
    det.morph(ims, dons, **kw)                                                                 # (captures and allocations out of the way)
    for colour, kernel in ((0.0, 'imm_morph_u8'), (1.0, 'imm_morph_colour_u8')):
        (plain, pm0), calls0 = _count_calls(ops, lambda: det.morph(ims, dons, colour=colour, return_transform=True, **kw))
        (none, pmn), callsn = _count_calls(ops, lambda: det.morph(ims, dons, colour=colour, mask=None, grow=3.0, mask_feather=0.5,
                                                                  return_transform=True, **kw))
        assert calls0 == callsn and calls0.count(kernel) == 2 and not [c for c in calls0 if 'hull' in c]
        assert all(torch.equal(x, y) for x, y in zip(plain, none))
        assert pmn.mask is None and pmn.hull_edges is None and pmn.hull_flags is None and pm0.hull_edges is None
        # with the mask: one imm_hull_fit per bucket behind imm_morph_poses, imm_morph_hull_u8 in place of the morph launch
        (out, pm), calls = _count_calls(ops, lambda: det.morph(ims, dons, colour=colour, mask='hull', return_transform=True, **kw))
        assert calls.count('imm_hull_fit') == 2 and calls.count('imm_morph_hull_u8') == 2 and kernel not in calls
        assert len(calls) == len(calls0) + 2
        assert [c for c in calls if c != 'imm_hull_fit'] == [c.replace(kernel, 'imm_morph_hull_u8') for c in calls0]
        assert all(calls[i - 1] == 'imm_morph_poses' for i, c in enumerate(calls) if c == 'imm_hull_fit')
        assert not all(torch.equal(x, y) for x, y in zip(plain, out))
        assert pm.mask == 'hull' and tuple(pm.hull_edges.shape) == (n, 10, 3) and pm.hull_edges.is_cuda and not pm.hull_flags.any()
        assert torch.equal(pm.flags, pm0.flags), 'hull_flags is OR-ed into nothing else'


def test_detector_morph_hull_against_the_restatement(ops, m128, scene):
    from imm_amd import keypoints as KP
    from imm_amd import morphing as MP
    cfg, model, eng, P, St = m128
    ims, dons, lm_a, lm_b = scene
    det = model.landmark_detector(S, max_batch=4)
    n = len(SURFACE_BOXES)
    assert len(plan_buckets(n, 4)) == 2
    rows, drows = KP.check_boxes(SURFACE_BOXES, len(ims)), KP.check_boxes(DONOR_BOXES, len(dons))
    shape = np.linspace(0.0, 1.0, n).astype(F32)
    texture = np.array([1.0, 0.3, 0.5, 1.0, 0.8, 0.6, 0.2], dtype=F32)
    sa, sb = CO.stats(ims, rows), CO.stats(dons, drows)
    for colour, grow, mf, feather, m, lam in ((0.0, 1.25, 0.1, 0.125, 2, 0.0),
                                              (1.0, np.linspace(0.8, 1.6, n).astype(F32), np.linspace(0.0, 0.3, n).astype(F32), 0.0, 0, 1e-2)):
        out, pm = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=shape, texture=texture, feather=feather, anchors=m, lam=lam,
                            landmarks=lm_a, donor_landmarks=lm_b, return_transform=True, colour=colour, mask='hull', grow=grow, mask_feather=mf)
        torch.cuda.synchronize()
        g, f = np.broadcast_to(np.asarray(grow, F32), (n,)), np.broadcast_to(np.asarray(mf, F32), (n,))
        poses = pm.poses.cpu().numpy()
        assert np.array_equal(poses.view(np.uint32), MP.blend_poses(lm_a, lm_b, shape).view(np.uint32))
        want, wflags = HR.hull_fit(poses, rows, g)
        edges = pm.hull_edges.cpu().numpy()
        assert edges.dtype == F32 and same_values(edges, want), 'PhotoMorph.hull_edges, bit for bit'
        assert np.array_equal(pm.hull_flags.cpu().numpy(), wflags) and not wflags.any() and not pm.flags.any()
        assert np.array_equal(pm.grow, g) and np.array_equal(pm.mask_feather, f) and np.array_equal(pm.inv_soft, HR.inv_soft(rows, f))
        for i in range(n):
            w = pm.hull_weight(i)
            assert w.dtype == F32 and np.array_equal(w, HR.weight_f32(want[i], pm.inv_soft[i], rows[i, 3] - rows[i, 1], rows[i, 4] - rows[i, 2]))
            assert (w > 0).mean() > 0.1 and 0.0 < w.max() <= 1.0 and w.min() == 0.0
        gain = None
        if colour:
            gain = pm.colour_gain.cpu().numpy()
            assert np.array_equal(gain.view(np.uint32), CO.gain(sa, sb, np.full(n, colour, F32), 2.0)[0].view(np.uint32))
        coef_a, coef_b, ctrl = pm.coef_a.cpu().numpy(), pm.coef_b.cpu().numpy(), pm.ctrl.cpu().numpy()
        ref64, covered = HR.morph_f64(ims, rows, dons, drows, ctrl, coef_a, coef_b, texture, WR.inv_ramp(rows, feather), edges, pm.inv_soft, gain)
        got = [o.cpu().numpy() for o in out]
        n_diff, worst, _near, n_cov = UR.within_cap(got, ref64, covered, WR.no_band(ims))
        plain = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=shape, texture=texture, feather=feather, anchors=m, lam=lam,
                          landmarks=lm_a, donor_landmarks=lm_b, colour=colour)
        n_box = sum(int(b.sum()) for b in CR.box_mask(ims, rows))
        moved = sum(int((x != p.cpu().numpy()).any(axis=2).sum()) for x, p in zip(got, plain))
        print('\nMORPH(mask=hull) colour=%g feather=%g anchors=%d lam=%g: %d of %d pixels with w > 0 differ from the f64 restatement (max %d); '
              '%d box pixels; %d differ from mask=None' % (colour, feather, m, lam, n_diff, n_cov, worst, n_box, moved))
        assert n_cov < n_box and moved > 0.1 * n_cov and all(np.array_equal(x[~c], im[~c]) for x, im, c in zip(got, ims, covered))
        # a second call gives the same bytes and leaves the first call's result alone
        before = [o.clone() for o in out]
        again = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=shape, texture=texture, feather=feather, anchors=m, lam=lam,
                          landmarks=lm_a, donor_landmarks=lm_b, colour=colour, mask='hull', grow=grow, mask_feather=mf)
        assert all(torch.equal(x, y) for x, y in zip(before, again)) and all(torch.equal(x, y) for x, y in zip(before, out))
    for kw, match in ((dict(mask='ellipse'), 'mask'), (dict(mask='hull', grow=0.0), 'grow'), (dict(mask='hull', grow=17.0), 'grow'),
                      (dict(grow=float('nan')), 'grow'), (dict(mask='hull', mask_feather=1.5), 'mask_feather'),
                      (dict(mask='hull', grow=[1.0] * 3), 'grow')):
        args = dict(photos=ims, donors=dons, boxes=SURFACE_BOXES, donor_boxes=DONOR_BOXES)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            det.morph(**args)
    # the photos handed in are not written
    assert all(np.array_equal(im, smooth_photo(h, w, 60 + i)) for i, (im, (h, w)) in enumerate(zip(ims, SURFACE_SIZES)))


def test_generate_script_morphs_with_the_mask(ops, m128, tmp_path, capsys):
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
    common = ['--configs', conf, '--checkpoint', ckpt, '--appearance-dir', imdir, '--boxes', boxes, '--batch-size', '4', '--morph',
              '--donor-dir', str(donor_dir), '--shape', '0.25', '--texture', '0.75', '--feather', '0.0']
    det = LandmarkDetector.from_checkpoint(load_configs([conf]).model, ckpt, image_size=S, max_batch=4, device=DEV)
    photos = [pixels[n] for n in names]
    api_rows = [(names.index(r[0]),) + r[1:] for r in rows]
    plain = det.morph(photos, [donor], api_rows, None, shape=0.25, texture=0.75, feather=0.0)
    for extra, kw in ((['--mask', 'hull'], dict(mask='hull')),
                      (['--mask', 'hull', '--grow', '4', '--mask-feather', '0.3', '--colour', '1'], dict(mask='hull', grow=4.0, mask_feather=0.3, colour=1.0))):
        out_dir = str(tmp_path / ('out%d' % len(extra)))
        _run_script(script, common + extra + ['--out-dir', out_dir])
        assert '2 faces morphed in 4 photos, 1 step ->' in capsys.readouterr().out
        want = det.morph(photos, [donor], api_rows, None, shape=0.25, texture=0.75, feather=0.0, **kw)
        for n, w in zip(names, want):
            png = np.asarray(Image.open(os.path.join(out_dir, n.replace('.jpg', '.png'))))
            assert np.array_equal(png, w.cpu().numpy()), n
        assert not all(torch.equal(w, p) for w, p in zip(want, plain)), 'the flag changes the picture'
    for extra, match in ((['--mask', 'hull', '--grow', '0'], 'grow'), (['--mask', 'hull', '--mask-feather', '2'], 'mask_feather')):
        with pytest.raises(ValueError, match=match):
            _run_script(script, common + extra + ['--out-dir', str(tmp_path / 'no')])
    with pytest.raises(ValueError, match='go with --morph'):
        _run_script(script, [a for a in common if a != '--morph'][:10] + ['--mask', 'hull', '--out-dir', str(tmp_path / 'no')])
