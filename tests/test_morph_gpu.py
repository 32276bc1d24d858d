"""Morph on the MI355X: imm_morph_poses bit for bit against blend_poses, imm_morph_u8 behind imm_morph_poses and ONE imm_warp_fit over
2 n rows within the cap of the f64 restatement of the rule (tests/morph_reference.py) driven by the kernel's own coefficients, texture 0
against imm_warp_u8 bit for bit, the identities bit for bit, invariance under splitting a call into launches, guarded buffers, and
LandmarkDetector.morph with the script."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compose_reference as CR                                               # noqa: E402
import guarded                                                               # noqa: E402
import morph_reference as R                                                  # noqa: E402
import unalign_reference as UR                                               # noqa: E402
import warp_reference as WR                                                  # noqa: E402
from alignment_reference import smooth_photo                                  # noqa: E402
from dataset_fixtures import make_celeba_tree                                 # noqa: E402
from test_detector_gpu import _run_script, _write_config                      # noqa: E402
from test_generator_gpu import make_model as make_generator_model             # noqa: E402
from test_unalign_gpu import SURFACE_BOXES, SURFACE_SIZES                     # noqa: E402
from test_warp_gpu import dev, run_fit, run_warp, ulp32                       # noqa: E402

from imm_amd import generation as G                                           # noqa: E402
from imm_amd import morphing as MP                                            # noqa: E402
from imm_amd import warping as WP                                             # noqa: E402
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


def same_values(a, b):
    """Equal bit for bit wherever neither is NaN, and NaN in the same places."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def run_poses(ops, mu_a, mu_b, shape, slack=0):
    """imm_morph_poses in guarded buffers -> (poses2, mu2) f32 [2, n, K, 2] as host arrays.  slack > 0: mu_a is the head of a larger
    buffer (as the pose head's is), whose tail holds NaN."""
    n, K = mu_a.shape[:2]
    guarded.reset()
    poses2, mu2 = guarded.out((2, n, K, 2), torch.float32, DEV), guarded.out((2, n, K, 2), torch.float32, DEV)
    big = np.full((n + slack, K, 2), np.nan, F32)
    big[:n] = mu_a
    a_d = guarded.inp(_t(big), DEV)[:n]
    ops.morph_poses(a_d, guarded.inp(_t(mu_b), DEV), guarded.inp(_t(np.asarray(shape, F32)), DEV), poses2, mu2)
    torch.cuda.synchronize()
    guarded.check_guards()
    return poses2.cpu().numpy(), mu2.cpu().numpy()


def device_fit(ops, mu_a, mu_b, shape, m, lam):
    """imm_morph_poses, then ONE imm_warp_fit over the 2 n rows -> (poses f32 [n, K, 2], coef_a, coef_b f32 [n, M + 3, 2], ctrl f32
    [n, M, 2], flags int32 [n], the OR of the two halves)."""
    n, K = mu_a.shape[:2]
    poses2, mu2 = run_poses(ops, mu_a, mu_b, shape)
    coef, ctrl, flags = run_fit(ops, poses2.reshape(2 * n, K, 2), mu2.reshape(2 * n, K, 2), m, 1.0, lam)
    assert np.array_equal(ctrl[:n].view(np.uint32), ctrl[n:].view(np.uint32)), 'the two splines share their control points'
    return poses2[0], coef[:n], coef[n:], ctrl[:n], flags[:n] | flags[n:]


def box_area(rows):
    a = (rows[:, 3].astype(np.int64) - rows[:, 1]) * (rows[:, 4].astype(np.int64) - rows[:, 2])
    return int(min(max(1, a.max()), 2 ** 31 - 1))


def run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, launches=None, links=None, donor_is_src=False,
              max_pixels=None, gain=None, edges=None, soft=None, ring=None, diff=None, seamless=None):
    """The paste over the packed photos, through the named wrapper of what is given: imm_morph_seam_u8 with ring f32 [n, B, 2], diff f32
    [n, B, 3] and seamless f32 [n], else imm_morph_hull_u8 with edges f32 [n, K, 3] and soft f32 [n], else imm_morph_colour_u8 with gain
    f32 [n, 3, 2] (the first two take a gain as well), else imm_morph_u8.  Source, donor, canvas and every array given in guarded buffers,
    the rows issued as the given launches (lists of consecutive row indices, in order; default: one launch of all rows), the grid sized
    by max_pixels (default: the launch's largest box).  donor_is_src: the donor buffer IS the source buffer (donors must be the photos).
    Returns (the whole canvas as a host array, the packed input)."""
    buf, offs, hw = CR.pack(photos)
    dbuf, doffs, dhw = CR.pack(donors)
    guarded.reset()
    src = guarded.inp(_t(buf), DEV)
    don = src if donor_is_src else guarded.inp(_t(dbuf), DEV)
    canvas = guarded.out(buf.shape, torch.uint8, DEV, fill=_t(buf))
    offs_d, hw_d, doffs_d, dhw_d = dev(ops, offs), dev(ops, hw), dev(ops, doffs), dev(ops, dhw)
    ctrl_d, ca_d, cb_d, tex_d, gain_d, edges_d, soft_d, ring_d, diff_d, seam_d = (
        None if a is None else guarded.inp(_t(np.asarray(a, F32)), DEV) for a in (ctrl, coef_a, coef_b, texture, gain, edges, soft, ring, diff, seamless))
    ramp = WR.inv_ramp(rows, feather)
    assert np.array_equal(ramp, G.compose_inv_ramp(rows, feather))
    for part in ([list(range(len(rows)))] if launches is None else launches):
        assert part == list(range(part[0], part[-1] + 1))
        sl = slice(part[0], part[-1] + 1)
        sub = rows[sl]
        lk = G.compose_links(sub) if links is None else links[sl]
        common = (src, canvas, offs_d, hw_d, don, doffs_d, dhw_d, dev(ops, sub), dev(ops, drows[sl]), dev(ops, lk), dev(ops, ramp[sl]), tex_d[sl],
                  ctrl_d[sl], ca_d[sl], cb_d[sl])
        area = box_area(sub) if max_pixels is None else max_pixels
        g = None if gain is None else gain_d[sl]
        if ring is not None:
            ops.morph_seam_u8(*common, g, edges_d[sl], soft_d[sl], ring_d[sl], diff_d[sl], seam_d[sl], area)
        elif edges is not None:
            ops.morph_hull_u8(*common, g, edges_d[sl], soft_d[sl], area)
        elif gain is not None:
            ops.morph_colour_u8(*common, g, area)
        else:
            ops.morph_u8(*common, area)
    torch.cuda.synchronize()
    guarded.check_guards()
    assert np.array_equal(src.cpu().numpy(), buf), 'the source buffer is read only'
    assert np.array_equal(don.cpu().numpy(), buf if donor_is_src else dbuf), 'the donor buffer is read only'
    return canvas.cpu().numpy(), buf


def packed_mask(masks):
    """Per-photo bool masks -> the bool mask of their bytes in the packed buffer (padding: False)."""
    inside, _o, _h = CR.pack([np.repeat(c[:, :, None], 3, axis=2).astype(np.uint8) for c in masks])
    return inside == 1                                                       # (the padding of that buffer holds 0xA5)


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the pose blend
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [3, 10, 64])
@pytest.mark.parametrize('n', [1, 3, 65])
def test_morph_poses_kernel(ops, n, K):
    rng = np.random.RandomState(100 * n + K)
    a, b = rng.uniform(-1, 1, (n, K, 2)).astype(F32), rng.uniform(-1, 1, (n, K, 2)).astype(F32)
    s = rng.uniform(0, 1, n).astype(F32)
    s[0] = 0.0 if n == 1 else s[0]
    if n > 1:
        s[1], s[2] = 0.0, 1.0
        a[0, K // 2, 1], b[0, 0, 0] = np.nan, np.nan
        a[1, 0, 0], b[2, 1, 1] = -0.0, 0.0
    for slack in (0, 5):
        poses2, mu2 = run_poses(ops, a, b, s, slack)
        want = MP.blend_poses(a, b, s)
        assert same_values(poses2[0], want) and same_values(poses2[1], want), 'poses2 is not blend_poses, twice, bit for bit'
        assert same_values(mu2[0], a) and same_values(mu2[1], b), 'mu2 is not (mu_a, mu_b)'
    if n > 1:
        assert np.array_equal(poses2[0, 1], a[1]) and np.array_equal(poses2[0, 2], b[2]), 'the end points give the inputs as values'
        assert np.isnan(poses2[0, 0, K // 2, 1]) and np.isnan(poses2[0, 0, 0, 0]) and np.isnan(poses2[0]).sum() == 2
    else:
        assert np.array_equal(poses2[0], a)
    # the other end alone
    poses2, _mu2 = run_poses(ops, a, b, np.ones(n, F32))
    ok = ~np.isnan(poses2[0])
    assert np.array_equal(poses2[0][ok], b[ok]) and (n == 1 or (~ok).sum() == 2)


# ----------------------------------------------------------------------------------------------------------------------------
# 2. the morph: parity and guards
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('feather', R.FEATHERS)
@pytest.mark.parametrize('K,m', R.KERNEL_SHAPES)
def test_morph_kernel_parity(ops, K, m, feather):
    photos, rows, donors, drows, mu_a, mu_b, shape, texture = R.kernel_case(K, m)
    for lam in R.LAMS:
        poses, coef_a, coef_b, ctrl, flags = device_fit(ops, mu_a, mu_b, shape, m, lam)
        assert flags.tolist() == [int(b == R.NAN_ROW) for b in range(len(rows))]
        assert same_values(poses, MP.blend_poses(mu_a, mu_b, shape))
        assert not coef_a[R.SHAPE_ZERO_ROW].any() and not coef_b[R.SHAPE_ONE_ROW].any(), 'a zero right-hand side: zero coefficients'
        got, buf = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather)
        ramp = WR.inv_ramp(rows, feather)
        ref64, covered = R.morph_f64(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ramp)
        ref32, _cov = R.morph_f32(photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, ramp)
        out = CR.unpack(got, photos)
        n32 = sum(int((a != b).any(axis=2).sum()) for a, b in zip(out, ref32))
        d64 = [np.abs(a.astype(int) - b.astype(int)).max(axis=2) for a, b in zip(out, ref64)]
        print('\nMORPH KERNEL K=%d anchors=%d lam=%g feather=%g: %d of %d covered pixels differ from the f64 restatement (max %d), %d from '
              'the f32 one' % (K, m, lam, feather, sum(int((d > 0).sum()) for d in d64), sum(int(c.sum()) for c in covered),
                               max(int(d.max()) for d in d64), n32))
        UR.within_cap(out, ref64, covered, WR.no_band(photos))
        # every byte no row writes - other pixels, the photo without a row, the padding between photos - is the input's
        inside = packed_mask(covered)
        assert inside.sum() == 3 * sum(int(c.sum()) for c in covered) and not covered[3].any()
        assert np.array_equal(got[~inside], buf[~inside])
        y0, x0, y1, x1 = rows[R.NAN_ROW, 1:]
        assert not covered[rows[R.NAN_ROW, 0]][y0:y1, x0:x1].any()
        changed = sum(int((o != p).any(axis=2).sum()) for o, p in zip(out, photos))
        assert changed > 0.3 * sum(int(c.sum()) for c in covered), 'the morph moves pixels'
    # the NaN row, the two bad-image rows, the bad-donor row (whose own box lies under row 4: the parity above would not tell its
    # silence from the mask) and the outside box write nothing, each alone in a launch and all of them together
    silent = sorted(R.SILENT_ROWS)
    assert len(silent) == 5
    for pick in [[b] for b in silent] + [silent]:
        got, buf = run_morph(ops, photos, rows[pick], donors, drows[pick], ctrl[pick], coef_a[pick], coef_b[pick], texture[pick], feather)
        assert np.array_equal(got, buf), pick


# ----------------------------------------------------------------------------------------------------------------------------
# 3. texture 0 is imm_warp_u8, 4. the identities
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,m', R.KERNEL_SHAPES)
def test_morph_texture_zero_is_the_warp(ops, K, m):
    photos, rows, donors, drows, mu_a, mu_b, shape, _texture = R.kernel_case(K, m)
    _poses, coef_a, coef_b, ctrl, _flags = device_fit(ops, mu_a, mu_b, shape, m, 0.0)
    good = [b for b in range(len(rows)) if b != R.NAN_ROW]
    assert np.isfinite(coef_b[good]).all()
    # imm_warp_u8 knows no donors: the row without a donor photo is taken out of its rows
    live = rows.copy()
    live[R.BAD_DONOR_ROW, 0] = -1
    for feather in R.FEATHERS:
        got, buf = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, np.zeros(len(rows), F32), feather)
        want, _buf = run_warp(ops, photos, live, ctrl, coef_a, feather)
        assert np.array_equal(got, want), feather
        assert not np.array_equal(got, buf)


@pytest.mark.parametrize('K,m', [(10, 0), (10, 2), (64, 4)])
def test_morph_identities(ops, K, m):
    photos, rows, donors, drows, mu_a, mu_b, shape, texture = R.kernel_case(K, m)
    n = len(rows)
    feathers = R.FEATHERS + (0.25,)
    # shape 0 and texture 0: coef_a is exactly zero, the donor counts for nothing
    zero = np.zeros(n, F32)
    _poses, coef_a, coef_b, ctrl, flags = device_fit(ops, mu_a, mu_b, zero, m, 0.0)
    good = [b for b in range(n) if b != R.NAN_ROW]
    assert not coef_a[good].any() and coef_b[good].any() and np.isfinite(coef_b[good]).all()
    for feather in feathers:
        got, buf = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, zero, feather)
        assert np.array_equal(got, buf), feather
    # the donor is the face itself: own photos (the SAME device buffer), own boxes, mu_b = mu_a, for any shape
    own_rows = rows.copy()
    own_rows[list(R.BAD_IMAGE_ROWS), 0] = 0                                    # (as donor rows these would only silence rows silent anyway)
    _poses, coef_a, coef_b, ctrl, flags = device_fit(ops, mu_a, mu_a, shape, m, 0.0)
    assert np.array_equal(coef_a[good].view(np.uint32), coef_b[good].view(np.uint32))
    for tex in (0.0, 0.37, 1.0):
        for feather in feathers:
            for same_buffer in (True, False):
                got, buf = run_morph(ops, photos, rows, photos, own_rows, ctrl, coef_a, coef_b, np.full(n, tex, F32), feather,
                                     donor_is_src=same_buffer)
                assert np.array_equal(got, buf), (tex, feather, same_buffer)
    # and the morph is no no-op
    _poses, coef_a, coef_b, ctrl, _flags = device_fit(ops, mu_a, mu_b, shape, m, 0.0)
    got, buf = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, 0.25)
    assert not np.array_equal(got, buf)


# ----------------------------------------------------------------------------------------------------------------------------
# 5. split invariance
# ----------------------------------------------------------------------------------------------------------------------------
def test_morph_split_invariance(ops):
    photos, rows, donors, drows, mu_a, mu_b, shape, texture = R.kernel_case(10, 2)
    _poses, coef_a, coef_b, ctrl, _flags = device_fit(ops, mu_a, mu_b, shape, 2, 0.0)
    n = len(rows)
    for feather in (0.0, 0.125):
        one, _ = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather)
        two, _ = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, [list(range(0, 4)), list(range(4, n))])
        each, _ = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, [[i] for i in range(n)])
        assert np.array_equal(one, two) and np.array_equal(one, each), feather
    # with a donor for row 6 as well, all three mutually overlapping rows are live: the same invariance, and the split parts them
    full = drows.copy()
    full[R.BAD_DONOR_ROW, 0] = 1
    one, _ = run_morph(ops, photos, rows, donors, full, ctrl, coef_a, coef_b, texture, 0.125)
    two, _ = run_morph(ops, photos, rows, donors, full, ctrl, coef_a, coef_b, texture, 0.125, [list(range(0, 4)), list(range(4, n))])
    each, _ = run_morph(ops, photos, rows, donors, full, ctrl, coef_a, coef_b, texture, 0.125, [[i] for i in range(n)])
    assert np.array_equal(one, two) and np.array_equal(one, each)
    live, _ = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, 0.125)
    assert not np.array_equal(one, live), 'row 6 writes once it has a donor'
    assert sum(i < 4 for i in WR.OVERLAPPING) == 1
    # their order matters
    ramp = WR.inv_ramp(rows, 0.0)
    fwd, _c = R.morph_f32(photos, rows, donors, full, ctrl, coef_a, coef_b, texture, ramp)
    order = [i for i in range(n) if i not in WR.OVERLAPPING] + list(WR.OVERLAPPING)[::-1]
    rev, _c = R.morph_f32(photos, rows[order], donors, full[order], ctrl[order], coef_a[order], coef_b[order], texture[order], ramp[order])
    assert not all(np.array_equal(a, b) for a, b in zip(fwd, rev))


def test_morph_one_block_per_row(ops):
    """The grid-size argument set to 1: ONE block of 256 threads per row carries every box through the grid-stride loop, and the bytes
    are those of a grid as large as the largest box."""
    photos, rows, donors, drows, mu_a, mu_b, shape, texture = R.kernel_case(10, 2)
    _poses, coef_a, coef_b, ctrl, _flags = device_fit(ops, mu_a, mu_b, shape, 2, 0.0)
    assert ((rows[:, 3] - rows[:, 1]) * (rows[:, 4] - rows[:, 2])).max() > 2 * 256
    for feather in (0.0, 0.125):
        full, _ = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather)
        one, _ = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, coef_b, texture, feather, max_pixels=1)
        assert np.array_equal(one, full), feather


# ----------------------------------------------------------------------------------------------------------------------------
# 6. guards: whatever the device buffers hold, nothing outside the two packed buffers is addressed
# ----------------------------------------------------------------------------------------------------------------------------
def test_morph_addresses_nothing_outside_the_photos(ops):
    photos, rows, donors, drows, mu_a, mu_b, shape, texture = R.kernel_case(10, 2)
    _poses, coef_a, coef_b, ctrl, _flags = device_fit(ops, mu_a, mu_b, shape, 2, 0.0)
    rng = np.random.RandomState(9)
    n = len(rows)

    def wild(coef):
        w = coef.copy()
        w[1::4] *= F32(1e6)                                 # samples far outside the photo: clamped to its edge
        w[2::4] *= F32(1e30)                                # beyond what an int holds
        w[3::4, 5] = np.inf
        w[0, 2, 1] = np.nan
        return w
    links = rng.randint(-5, n + 5, size=(n, 2)).astype(np.int32)             # chains that loop, leave [0, n) and join other photos
    far = drows.copy()
    far[0::3, 1:] += np.array([100000, -70000, 100000, -70000], dtype=np.int32)            # donor boxes far outside their photos
    far[1, 1:] = (-(1 << 23), -(1 << 23), 1 << 23, 1 << 23)                             # a donor box of 2^24 pixels a side
    boxes = packed_mask(CR.box_mask(photos, rows[[b for b in range(n) if 0 <= rows[b, 0] < len(photos)]]))
    for ca, cb in ((wild(coef_a), coef_b), (coef_a, wild(coef_b)), (wild(coef_a), wild(coef_b))):
        for lk in (None, links):
            for dr in (drows, far):
                got, buf = run_morph(ops, photos, rows, donors, dr, ctrl, ca, cb, texture, 0.125, links=lk)   # checks every guard band
                assert np.array_equal(got[~boxes], buf[~boxes])
    # finite coefficients and far donor boxes: the taps are clamped to the donor photo's edge, the rows still write
    # (without the 2^24 box, where an f32 place is a pixel coarse)
    far[1] = drows[1]
    got, buf = run_morph(ops, photos, rows, donors, far, ctrl, coef_a, coef_b, texture, 0.125)
    ref64, covered = R.morph_f64(photos, rows, donors, far, ctrl, coef_a, coef_b, texture, WR.inv_ramp(rows, 0.125))
    UR.within_cap(CR.unpack(got, photos), ref64, covered, WR.no_band(photos))
    # NaN coefficients on one side only: that row writes nothing, whatever the other side and the texture are
    for side in (0, 1):
        for tex in (0.0, 1.0):
            nan_a, nan_b = (np.full_like(coef_a, np.nan), coef_b) if side == 0 else (coef_a, np.full_like(coef_b, np.nan))
            got, buf = run_morph(ops, photos, rows, donors, drows, ctrl, nan_a, nan_b, np.full(n, tex, F32), 0.0)
            assert np.array_equal(got, buf), (side, tex)
    # one row's donor side NaN: the others write as before, that row's box keeps what the rows under it left
    b = 2
    part = coef_b.copy()
    part[b] = np.nan
    got, _buf = run_morph(ops, photos, rows, donors, drows, ctrl, coef_a, part, texture, 0.125)
    off = drows.copy()
    off[b, 0] = -1
    want, _buf = run_morph(ops, photos, rows, donors, off, ctrl, coef_a, coef_b, texture, 0.125)
    assert np.array_equal(got, want)


# ----------------------------------------------------------------------------------------------------------------------------
# 7. LandmarkDetector.morph
# ----------------------------------------------------------------------------------------------------------------------------
DONOR_SIZES = [(70, 88), (96, 64), (81, 81)]
DONOR_BOXES = [(0, 3, 5, 66, 80), (1, 10, 2, 90, 60), (2, 0, 0, 81, 81), (0, -5, 20, 60, 95), (2, 8, 12, 70, 66), (1, 30, 6, 96, 58), (0, 2, 2, 50, 70)]


@pytest.fixture(scope='module')
def m128(ops):
    return make_generator_model(10, S, 4)


@pytest.fixture(scope='module')
def scene():
    """Seven rows over six photos, one overlap, two buckets at max_batch = 4 (test_unalign_gpu's scene), seven donor rows over three
    donor photos of other sizes, and landmarks for both sides on a jittered grid (an untrained model's own landmarks sit in a small
    cloud, whose splines are too ill-conditioned for an f32 evaluation: DESIGN.md, Warp)."""
    ims = [smooth_photo(h, w, 60 + i) for i, (h, w) in enumerate(SURFACE_SIZES)]
    dons = [smooth_photo(h, w, 80 + i) for i, (h, w) in enumerate(DONOR_SIZES)]
    lm_a, lm_b = R.landmarks(10, len(SURFACE_BOXES), np.random.RandomState(12))
    return ims, dons, lm_a, lm_b


def test_detector_morph_against_the_restatement(m128, scene):
    from imm_amd import keypoints as KP
    cfg, model, eng, P, St = m128
    ims, dons, lm_a, lm_b = scene
    det = model.landmark_detector(S, max_batch=4)
    n = len(SURFACE_BOXES)
    assert len(plan_buckets(n, 4)) == 2
    rows, drows = KP.check_boxes(SURFACE_BOXES, len(ims)), KP.check_boxes(DONOR_BOXES, len(dons))
    detected = det.detect(torch.from_numpy(np.stack([smooth_photo(S, S, 5)]).astype(F32)))
    warped = det.warp(ims, lm_a, SURFACE_BOXES, lam=1.0)
    shape = np.linspace(0.0, 1.0, n).astype(F32)
    texture = np.array([1.0, 0.3, 0.5, 0.0, 0.8, 0.6, 0.2], dtype=F32)
    for feather, m, lam in ((0.125, 2, 0.0), (0.0, 0, 1e-2)):
        out, pm = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=shape, texture=texture, feather=feather, anchors=m, lam=lam,
                            landmarks=lm_a, donor_landmarks=lm_b, return_transform=True)
        torch.cuda.synchronize()
        assert isinstance(pm, MP.PhotoMorph) and (pm.anchors, pm.lam) == (m, lam)
        assert np.array_equal(pm.rows, rows) and np.array_equal(pm.donor_rows, drows)
        assert np.array_equal(pm.shape, shape) and np.array_equal(pm.texture, texture) and not pm.flags.any()
        assert torch.equal(pm.mu.cpu(), torch.from_numpy(lm_a)) and torch.equal(pm.donor_mu.cpu(), torch.from_numpy(lm_b))
        poses = pm.poses.cpu().numpy()
        assert np.array_equal(poses.view(np.uint32), MP.blend_poses(lm_a, lm_b, shape).view(np.uint32))
        coef_a, coef_b, ctrl = pm.coef_a.cpu().numpy(), pm.coef_b.cpu().numpy(), pm.ctrl.cpu().numpy()
        assert coef_a.shape == coef_b.shape == (n, 10 + 4 * m + 3, 2) and np.array_equal(ctrl, WP.control_points(poses, m))
        want_a, want_b, _c, _f, cond = R.fit2_f64(lm_a, lm_b, poses, m, lam)
        assert cond.max() <= 1e4
        for coef, want in ((coef_a, want_a), (coef_b, want_b)):
            assert (np.abs(coef - want) <= ulp32(want) + 1e-9 * np.abs(want).max(axis=1, keepdims=True)).all()
        ref64, covered = R.morph_f64(ims, rows, dons, drows, ctrl, coef_a, coef_b, texture, WR.inv_ramp(rows, feather))
        got = [o.cpu().numpy() for o in out]
        for o, im in zip(out, ims):
            assert o.dtype == torch.uint8 and o.device.type == 'cuda' and tuple(o.shape) == im.shape
        n_diff, worst, _near, n_cov = UR.within_cap(got, ref64, covered, WR.no_band(ims))
        changed = sum(int((g != im).any(axis=2).sum()) for g, im in zip(got, ims))
        print('\nMORPH() feather=%g anchors=%d lam=%g: %d of %d covered pixels differ from the f64 restatement (max %d), %d changed' % (
            feather, m, lam, n_diff, n_cov, worst, changed))
        assert changed > 0.3 * n_cov and all(np.array_equal(g[~c], im[~c]) for g, im, c in zip(got, ims, covered))
        # a second call gives the same bytes and leaves the first call's result alone
        before = [o.clone() for o in out]
        again = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=shape, texture=texture, feather=feather, anchors=m, lam=lam,
                          landmarks=lm_a, donor_landmarks=lm_b)
        assert all(torch.equal(x, y) for x, y in zip(before, again)) and all(torch.equal(x, y) for x, y in zip(before, out))
        if lam == 0.0:
            # the blended landmarks, in photo pixels, lead to the own landmarks in the photo and the donor's in the donor box
            px = lambda q, rw: rw[:, None, 1:3] + (np.asarray(q, np.float64) + 1.0) * ((rw[:, None, 3:5] - rw[:, None, 1:3]) / 2.0)
            assert np.abs(pm.to_source(px(poses, rows)) - px(lm_a, rows)).max() < 1e-3
            assert np.abs(pm.to_donor(px(poses, rows)) - px(lm_b, drows)).max() < 1e-3
    # one donor row for all faces, scalar shape, texture = shape by default, whole-photo boxes by default
    one, pm1 = det.morph(ims, dons[:1], SURFACE_BOXES, [(0, 3, 5, 66, 80)], shape=0.25, landmarks=lm_a, donor_landmarks=lm_b[:1],
                         return_transform=True)
    assert pm1.donor_rows.tolist() == [[0, 3, 5, 66, 80]] * n and pm1.shape.tolist() == [0.25] * n == pm1.texture.tolist()
    assert torch.equal(pm1.donor_mu.cpu(), torch.from_numpy(lm_b[:1]).expand(n, 10, 2))
    whole = det.morph(ims, dons[:1], shape=0.5, landmarks=lm_a[:6], donor_landmarks=lm_b[:1])
    assert len(whole) == 6 and all(tuple(o.shape) == im.shape for o, im in zip(whole, ims))
    # detect and warp are what they were
    assert torch.equal(detected, det.detect(torch.from_numpy(np.stack([smooth_photo(S, S, 5)]).astype(F32))))
    assert all(torch.equal(x, y) for x, y in zip(warped, det.warp(ims, lm_a, SURFACE_BOXES, lam=1.0)))
    # the photos handed in are not written
    assert all(np.array_equal(im, smooth_photo(h, w, 60 + i)) for i, (im, (h, w)) in enumerate(zip(ims, SURFACE_SIZES)))
    assert all(np.array_equal(im, smooth_photo(h, w, 80 + i)) for i, (im, (h, w)) in enumerate(zip(dons, DONOR_SIZES)))


def test_detector_morph_with_its_own_landmarks(m128, scene):
    """Without landmarks= / donor_landmarks=: both pose programs run.  warp() finds a face's own landmarks itself, so texture = 0 is
    compared with it here, with the model's landmarks on the own side and the donors' on the grid (shape near 1 keeps the blended
    control points apart; the comparison is byte for byte, whatever the conditioning)."""
    from imm_amd.inference import LandmarkDetector
    cfg, model, eng, P, St = m128
    ims, dons, lm_a, lm_b = scene
    det = model.landmark_detector(S, max_batch=4)
    n = len(SURFACE_BOXES)
    mu, dmu = det.landmarks(ims, SURFACE_BOXES), det.landmarks(dons, DONOR_BOXES)
    shape = np.linspace(0.1, 0.9, n).astype(F32)
    out, pm = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=shape, lam=1.0, return_transform=True)
    assert torch.equal(pm.mu, mu) and torch.equal(pm.donor_mu, dmu), 'the landmarks are detector.landmarks, bit for bit'
    want = MP.blend_poses(mu.cpu().numpy(), dmu.cpu().numpy(), shape)
    assert np.array_equal(pm.poses.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert not all(np.array_equal(o.cpu().numpy(), im) for o, im in zip(out, ims))
    # plain launches give the same bytes
    plain = LandmarkDetector(model, S, max_batch=4, use_graph=False)
    assert all(torch.equal(x, y) for x, y in zip(plain.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=shape, lam=1.0), out))
    # shape 0 and texture 0: the photos, bit for bit
    same = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=0.0, texture=0.0)
    assert all(np.array_equal(o.cpu().numpy(), im) for o, im in zip(same, ims))
    # texture 0 is warp() towards the blended pose
    shape = np.linspace(0.7, 1.0, n).astype(F32)
    for feather, m in ((0.125, 2), (0.0, 0)):
        out, pm = det.morph(ims, dons, SURFACE_BOXES, DONOR_BOXES, shape=shape, texture=0.0, feather=feather, anchors=m, donor_landmarks=lm_b,
                            return_transform=True)
        assert not pm.flags.any() and bool(torch.isfinite(pm.coef_b).all()) and not pm.coef_b[n - 1].any()
        want, pw = det.warp(ims, pm.poses, SURFACE_BOXES, feather=feather, anchors=m, return_transform=True)
        assert torch.equal(pw.coef, pm.coef_a) and torch.equal(pw.ctrl, pm.ctrl)
        assert all(torch.equal(x, y) for x, y in zip(out, want))
        assert not all(np.array_equal(o.cpu().numpy(), im) for o, im in zip(out, ims))


def test_detector_morph_issues_the_parents_calls(ops, m128, scene):
    """The library calls of one morph() call on the module's scene (seven rows, buckets of 4 and 3), by name and in order, against the lists
    recorded from the commit in front of ops.morph_paste (landmarks given to both sides; in the last case the own side is staged and
    runs its captured program), and the tensors handed to _join: everything on the device that the call returns, the PhotoMorph's
    tensors and the photos' packed buffer, is among them, so the allocator cannot hand a result out again while the detector's stream
    still works on it."""
    from test_colour_gpu import _count_calls
    cfg, model, eng, P, St = m128
    ims, dons, lm_a, lm_b = scene
    det = model.landmark_detector(S, max_batch=4)
    n = len(SURFACE_BOXES)
    assert [count for _s, count, _b in plan_buckets(n, 4)] == [4, 3]
    base = dict(boxes=SURFACE_BOXES, donor_boxes=DONOR_BOXES, shape=np.linspace(0.0, 1.0, n).astype(F32), texture=0.8, donor_landmarks=lm_b,
                return_transform=True)
    hull, seam = dict(mask='hull'), dict(mask='hull', seamless=1.0, ring=16)
    stats = ['imm_colour_stats_u8', 'imm_colour_stats_u8', 'imm_colour_gain']
    cases = [
        (dict(colour=0.0), ['imm_morph_poses', 'imm_warp_fit', 'imm_morph_u8'] * 2),
        (dict(colour=0.0, **hull), ['imm_morph_poses', 'imm_hull_fit', 'imm_warp_fit', 'imm_morph_hull_u8'] * 2),
        (dict(colour=0.0, **seam), ['imm_morph_poses', 'imm_hull_fit', 'imm_warp_fit', 'imm_seam_fit', 'imm_morph_seam_u8'] * 2),
        (dict(colour=1.0), stats + ['imm_morph_poses', 'imm_warp_fit', 'imm_morph_colour_u8'] * 2),
        (dict(colour=1.0, **hull), stats + ['imm_morph_poses', 'imm_hull_fit', 'imm_warp_fit', 'imm_morph_hull_u8'] * 2),
        (dict(colour=1.0, **seam), stats + ['imm_morph_poses', 'imm_hull_fit', 'imm_warp_fit', 'imm_seam_fit', 'imm_morph_seam_u8'] * 2),
        (dict(landmarks=None), ['imm_resize_crop_u8', 'imm_graph_launch', 'imm_morph_poses', 'imm_warp_fit', 'imm_morph_u8'] * 2)]
    for kw, want in cases:
        kw = dict(base, **dict(dict(landmarks=lm_a), **kw))
        det.morph(ims, dons, **kw)                                             # (captures and allocations out of the way)
        recorded, join0 = [], det._join
        det._join = lambda cur, *record: (recorded.extend(t.data_ptr() for t in record if t is not None), join0(cur, *record))[1]
        try:
            (out, pm), calls = _count_calls(ops, lambda: det.morph(ims, dons, **kw))
        finally:
            del det._join
        assert calls == want, kw
        held = [getattr(pm, a) for a in ('coef_a', 'coef_b', 'ctrl', 'mu', 'donor_mu', 'poses', 'flags', 'colour_gain', 'colour_flags',
                                         'hull_edges', 'hull_flags', 'seam_ring', 'seam_diff', 'seam_flags')]
        assert sum(t is not None for t in held) == 7 + 2 * (kw.get('colour', 0.0) > 0) + 2 * ('mask' in kw) + 3 * ('ring' in kw)
        assert all(t.is_cuda and t.data_ptr() in recorded for t in held if t is not None), kw
        assert min(o.data_ptr() for o in out) in recorded, 'the packed buffer of the photos returned'


def test_detector_morph_refusals(m128, scene):
    cfg, model, eng, P, St = m128
    ims, dons, lm_a, lm_b = scene
    det = model.landmark_detector(S, max_batch=4)
    for kw, match in ((dict(feather=0.75), 'feather'), (dict(anchors=18), '<= 80 control points'), (dict(anchors=-2), 'anchors'),
                      (dict(lam=-1.0), 'lam'), (dict(lam=float('nan')), 'lam'), (dict(shape=1.25), 'shape'), (dict(shape=float('nan')), 'shape'),
                      (dict(shape=[0.5] * 3), 'shape'), (dict(texture=-0.5), 'texture'), (dict(texture=[0.5] * 8), 'texture'),
                      (dict(donor_boxes=DONOR_BOXES[:3]), '3 donors for 7 faces'), (dict(donors=dons[:2], donor_boxes=None), '2 donors for 7 faces'),
                      (dict(donors=torch.zeros(3, S, S, 3)), 'u8 arrays'), (dict(photos=torch.zeros(6, S, S, 3)), 'u8 arrays'),
                      (dict(boxes=[(9, 0, 0, 5, 5)] * 7), 'names image'), (dict(donor_boxes=[(3, 0, 0, 5, 5)] * 7), 'names image'),
                      (dict(landmarks=lm_a[:3]), 'landmarks must be'), (dict(donor_landmarks=lm_b[:, :9]), 'donor_landmarks must be'),
                      (dict(landmarks=np.full_like(lm_a, np.inf)), 'finite')):
        args = dict(photos=ims, donors=dons, boxes=SURFACE_BOXES, donor_boxes=DONOR_BOXES)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            det.morph(**args)


def test_generate_script_morphs_photos(m128, tmp_path, capsys):
    from PIL import Image
    from imm_amd.inference import LandmarkDetector
    from imm_amd.utils.config import load_configs
    cfg, model, eng, P, St = m128
    root = str(tmp_path / 'celeba')
    names, pixels = make_celeba_tree(root, n=6)
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, ckpt)
    conf = _write_config(tmp_path, root, str(tmp_path / 'logs'))
    imdir = os.path.join(root, 'Img', 'img_align_celeba_hq')
    rows = [(names[0], 20, 10, 180, 150), (names[2], -10, 30, 120, 170), (names[0], 100, 60, 215, 175), (names[5], 0, 0, 150, 100)]
    boxes = str(tmp_path / 'faces.csv')
    with open(boxes, 'w') as f:
        f.write('file,y0,x0,y1,x1\n' + ''.join('%s,%d,%d,%d,%d\n' % r for r in rows))
    donor_dir = tmp_path / 'donors'
    donor_dir.mkdir()
    dnames, donors = ['a.png', 'b.png'], [smooth_photo(120, 100, 3), smooth_photo(90, 140, 4)]
    for nm, im in zip(dnames, donors):
        Image.fromarray(im).save(str(donor_dir / nm))
    drows = [('b.png', 5, 5, 85, 120), ('a.png', 0, 10, 110, 95), ('a.png', 20, 0, 120, 80), ('b.png', -5, 30, 80, 145)]
    dboxes = str(tmp_path / 'donors.csv')
    with open(dboxes, 'w') as f:
        f.write('file,y0,x0,y1,x1\n' + ''.join('%s,%d,%d,%d,%d\n' % r for r in drows))
    script = os.path.join(ROOT, 'scripts', 'generate.py')
    common = ['--configs', conf, '--checkpoint', ckpt, '--appearance-dir', imdir, '--boxes', boxes, '--batch-size', '4', '--morph',
              '--donor-dir', str(donor_dir), '--donor-boxes', dboxes]
    det = LandmarkDetector.from_checkpoint(load_configs([conf]).model, ckpt, image_size=S, max_batch=4, device=DEV)
    photos = [pixels[n] for n in names]
    api_rows = [(names.index(r[0]),) + r[1:] for r in rows]
    api_drows = [(dnames.index(r[0]),) + r[1:] for r in drows]
    pngs = [n.replace('.jpg', '.png') for n in names]
    # one morph
    out_dir = str(tmp_path / 'one')
    _run_script(script, common + ['--shape', '0.25', '--texture', '0.75', '--feather', '0.0', '--out-dir', out_dir])
    assert '4 faces morphed in 6 photos, 1 step ->' in capsys.readouterr().out
    assert sorted(os.listdir(out_dir)) == pngs
    want = det.morph(photos, donors, api_rows, api_drows, shape=0.25, texture=0.75, feather=0.0)
    for n, w in zip(names, want):
        png = np.asarray(Image.open(os.path.join(out_dir, n.replace('.jpg', '.png'))))
        assert np.array_equal(png, w.cpu().numpy()), n
        assert n in (names[0], names[2], names[5]) or np.array_equal(png, pixels[n]), n
    assert not all(np.array_equal(w.cpu().numpy(), pixels[n]) for n, w in zip(names, want)), 'the morph changes the photos with faces'
    # a sequence of three
    out_dir = str(tmp_path / 'seq')
    _run_script(script, common + ['--steps', '3', '--out-dir', out_dir])
    assert '4 faces morphed in 6 photos, 3 steps ->' in capsys.readouterr().out
    assert sorted(os.listdir(out_dir)) == ['000', '001', '002']
    for i, t in enumerate((0.0, 0.5, 1.0)):
        assert sorted(os.listdir(os.path.join(out_dir, '%03d' % i))) == pngs
        want = det.morph(photos, donors, api_rows, api_drows, shape=t, texture=t)
        for n, w in zip(names, want):
            png = np.asarray(Image.open(os.path.join(out_dir, '%03d' % i, n.replace('.jpg', '.png'))))
            assert np.array_equal(png, w.cpu().numpy()), (i, n)
            assert i > 0 or np.array_equal(png, pixels[n]), 'step 0 is the photo itself'
    for extra, match in ((['--warp'], 'do not go with it'), (['--steps', '1'], 'at least 2')):
        with pytest.raises(ValueError, match=match):
            _run_script(script, common + extra + ['--out-dir', str(tmp_path / 'no')])
    with pytest.raises(ValueError, match='go with --morph'):
        _run_script(script, [a for a in common if a != '--morph'] + ['--out-dir', str(tmp_path / 'no')])
