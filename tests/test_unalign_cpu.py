"""Unalign, host side (no GPU): the ABI of imm_unalign_maps / imm_unalign_u8 and their argument validation, the numpy restatements of
the pixel rule (tests/unalign_reference.py) against Alignment's point maps and against each other, the properties of the kernel case,
and the refusals of LandmarkDetector.unalign and ImageGenerator.repose(template=) that need no device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unalign_reference as R                                              # noqa: E402

from imm_amd import alignment as AL                                         # noqa: E402
from imm_amd import generation as G                                         # noqa: E402
from imm_amd import inference as INF                                        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = R.S_KERNEL
FEATHERS = (0.0, 0.125, 0.5)


def template(K=5, image_size=128, seed=0):
    return AL.LandmarkTemplate(np.random.RandomState(seed).uniform(-0.8, 0.8, size=(K, 2)), image_size)


# ----------------------------------------------------------------------------------------------------------------------------
# ABI and validation
# ----------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_unalign_entry_points():
    from imm_amd import _lib as L
    assert L.ABI_VERSION >= 27
    assert L.symbols('imm_unalign.h') == ['imm_unalign_maps', 'imm_unalign_u8']


def test_unalign_validates_its_arguments_without_a_device():
    from imm_amd import _lib as L
    lib = L.load()
    one = C.c_void_p(16)                                   # a non-null pointer that is never read: validation comes first
    good = [one, one, one, one, 1, 1, 16, 16, one, one, None]
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (8, None), (9, None),                  # null pointers
                   (4, 0), (5, 0), (6, 0), (6, 8193), (7, 0), (7, 8193)):                              # n_images, n, image_size, out_size
        args = list(good)
        args[i] = bad
        assert lib.imm_unalign_maps(*args) == -1, (i, bad)
        assert b'unalign_maps' in lib.imm_last_error()
    good = [one, one, one, 1, one, one, one, one, 2.0, one, 3, 1, 16, 256, None]
    for i, bad in ((0, None), (1, None), (2, None), (4, None), (5, None), (6, None), (7, None), (9, None),            # null pointers
                   (3, 0), (8, 0.0), (8, -1.0), (8, float('nan')), (8, float('inf')), (10, 2), (11, 0), (11, 65536),    # n_images, inv_ramp, ld, n
                   (12, 0), (12, 8193), (13, 0)):                                                                     # out_size, max_pixels
        args = list(good)
        args[i] = bad
        assert lib.imm_unalign_u8(*args) == -1, (i, bad)
        assert b'unalign_u8' in lib.imm_last_error()


# ----------------------------------------------------------------------------------------------------------------------------
# the maps
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', ['similarity', 'affine'])
def test_maps_f64_inverts_what_to_source_maps(model):
    """B, t of the header against Alignment.to_source, and the f32 forward map against it within the bound that the f32 rounding of
    the six coefficients gives: |df| <= 4 * 2^-24 * (|m.0| r + |m.1| c + |m.2|) (each coefficient is off by at most 2^-24 of itself;
    the factor 4 leaves room for the f64 arithmetic on either side)."""
    rng = np.random.RandomState(3)
    n, Si, So = 9, 128, 96
    tpl = template(6, Si)
    mu = np.stack([tpl.points @ (s * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])).T + rng.uniform(-0.2, 0.2, 2)
                   + rng.standard_normal(tpl.points.shape) * (0.05 if model == 'affine' else 0.0)
                   for a, s in zip(rng.uniform(-1.2, 1.2, n), rng.uniform(0.5, 1.4, n))])
    coef = tpl.fit(mu, model).astype(np.float32)
    geom = np.stack([rng.randint(-40, 200, n), rng.randint(-40, 200, n), rng.uniform(0.4, 3.0, n), rng.uniform(0.4, 3.0, n)], axis=1)
    geom = geom.astype(np.float32)
    al = AL.Alignment(coef, geom, mu.astype(np.float32), model, 0.0, tpl, So)           # seven positional arguments still do
    assert al.rows is None
    img, hw = np.zeros(n, np.int64), np.array([[4000, 4000]])
    fwd, bbox, B, t = R.maps_f64(coef, geom, img, hw, Si, So)
    assert np.isfinite(fwd).all()
    pts = np.array([[0.0, 0.0], [So - 1.0, 0.0], [0.0, So - 1.0], [So - 1.0, So - 1.0], [So / 3.0, So / 1.7], [12.25, 80.5]])
    src = al.to_source(pts)                                                            # [n, P, 2]
    lin = np.einsum('nab,pb->npa', B, pts) + t[:, None]
    assert np.abs(src - lin).max() <= 1e-9 * max(1.0, np.abs(src).max())
    m = fwd.astype(np.float32).astype(np.float64)
    r, c = src[..., 0], src[..., 1]
    worst = 0.0
    for k, col in enumerate((0, 1)):
        got = m[:, None, 3 * k] * r + m[:, None, 3 * k + 1] * c + m[:, None, 3 * k + 2]
        bound = 4.0 * 2.0 ** -24 * (np.abs(m[:, None, 3 * k] * r) + np.abs(m[:, None, 3 * k + 1] * c) + np.abs(m[:, None, 3 * k + 2]))
        err = np.abs(got - pts[None, :, col])
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (k, float(err.max()), float(bound.min()))
    print('\nUNALIGN MAPS %s: round trip at most %.3f of the bound' % (model, worst))
    # and it is Alignment.to_aligned's map
    back = al.to_aligned(src)
    assert np.abs(back - pts[None]).max() < 1e-8
    # the bbox holds the corners
    for b in range(n):
        y0, x0, y1, x1 = bbox[b]
        cy, cx = src[b, :4, 0], src[b, :4, 1]
        assert y1 > y0 and x1 > x0
        assert y0 <= max(cy.min(), 0) and x0 <= max(cx.min(), 0) and y1 > min(cy.max(), 3999) and x1 > min(cx.max(), 3999)


def test_maps_of_the_kernel_case():
    photos, boxes, coef, geom, faces = R.kernel_case()
    hw = R.hw_of(photos)
    fwd, bbox, B, t = R.maps_f64(coef, geom, boxes[:, 0], hw, S, S)
    bad = [R.SINGULAR_ROW] + list(R.BAD_IMAGE_ROWS)
    assert np.isnan(fwd[bad]).all() and not bbox[bad].any()
    good = [b for b in range(len(boxes)) if b not in bad]
    assert np.isfinite(fwd[good]).all()
    assert not bbox[R.OUTSIDE_ROW].any(), 'a row wholly outside its photo has an empty bbox'
    # the maps are what the case says they are, up to the f32 rounding of coef
    for b in good:
        Bw, tw = R.KERNEL_MAPS[b][1]
        assert np.abs(B[b] - Bw).max() < 1e-6 and np.abs(t[b] - tw).max() < 1e-4, b
    dets = B[:, 0, 0] * B[:, 1, 1] - B[:, 0, 1] * B[:, 1, 0]
    assert dets[R.SINGULAR_ROW] == 0.0 and dets[6] < 0 and abs(dets[7] - 1.8 ** 2) < 1e-5 and abs(dets[2] - 0.16) < 1e-5
    # the translation row is exact
    assert np.array_equal(fwd[R.TRANSLATION_ROW], [1.0, 0.0, -3.0, 0.0, 1.0, -5.0])
    assert bbox[R.TRANSLATION_ROW].tolist() == [2, 4, 20, 22]
    # every bbox holds every pixel its row covers, and is clipped to the photo
    _out, covers = R.unalign_f32(photos, boxes[:, 0], fwd.astype(np.float32), faces, AL.unalign_inv_ramp(0.0, S), S, return_cover=True)
    for b in good:
        y0, x0, y1, x1 = bbox[b]
        outside = covers[b].copy()
        outside[y0:y1, x0:x1] = False
        assert not outside.any(), b
        assert 0 <= y0 <= y1 <= hw[boxes[b, 0], 0] and 0 <= x0 <= x1 <= hw[boxes[b, 0], 1]
        assert covers[b].any() == (b != R.OUTSIDE_ROW)
    # three rows overlap on one photo, out of spatial order, rows of other photos between them
    i, j, k = R.OVERLAPPING
    assert (covers[i] & covers[j] & covers[k]).sum() > 10 and boxes[[i, j, k], 0].tolist() == [1, 1, 1]
    assert boxes[i + 1, 0] != 1 and boxes[j + 1, 0] != 1
    # rows that reach over an edge or a corner of their photo
    assert covers[7][0].any() and covers[7][-1].any() and covers[8][-1, 0]
    assert not any(c is not None and c.any() for c in [covers[b] for b in bad])


# ----------------------------------------------------------------------------------------------------------------------------
# the two restatements
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ld', [3, 12])
@pytest.mark.parametrize('feather', FEATHERS)
def test_f32_restatement_against_f64(feather, ld):
    photos, boxes, coef, geom, faces = R.kernel_case(ld=ld)
    fwd, bbox, B, t = R.maps_f64(coef, geom, boxes[:, 0], R.hw_of(photos), S, S)
    inv = AL.unalign_inv_ramp(feather, S)
    a, covers = R.unalign_f32(photos, boxes[:, 0], fwd.astype(np.float32), faces, inv, S, return_cover=True)
    b, covered, near = R.unalign_f64(photos, boxes[:, 0], B, t, faces, inv, S)
    n_diff, worst, n_near, n_cov = R.within_cap(a, b, covered, near)
    print('\nUNALIGN f32 vs f64 feather=%g ld=%d: %d of %d covered pixels differ (max %d), %d in the border band' % (
        feather, ld, n_diff, n_cov, worst, n_near))
    # the coverage itself agrees outside the band
    for i, (m, nr) in enumerate(zip(covered, near)):
        mine = np.zeros_like(m)
        for bb, c in enumerate(covers):
            if c is not None and boxes[bb, 0] == i:
                mine |= c
        assert np.array_equal(mine & ~nr, m & ~nr)
    for x, y, p, m in zip(a, b, photos, covered):
        assert np.array_equal(y[~m], p[~m])                                            # nothing outside a quad moves
    assert np.array_equal(a[3], photos[3]) and not covered[3].any()                    # the photo without a row
    changed = sum(int((x != p).any(axis=2).sum()) for x, p in zip(a, photos))
    assert changed > 0.5 * n_cov                                                       # the faces did land


def test_identity_with_the_float_crop_returns_the_photo():
    rng = np.random.RandomState(1)
    photo = rng.randint(0, 256, size=(31, 45, 3)).astype(np.uint8)
    coef, geom = R.coefficients_of(np.eye(2), np.array([7.0, 11.0]), S, S)
    assert np.array_equal(coef, [[0, 0], [1, 0], [0, 1]]) and np.array_equal(geom, [7, 11, 1, 1])
    fwd, bbox, _B, _t = R.maps_f64(coef[None], geom[None], [0], [[31, 45]], S, S)
    faces = R.float_crop(photo, 7, 11, S)[None]
    for feather in (0.0, 0.1, 0.25, 0.5):
        out = R.unalign_f32([photo], [0], fwd.astype(np.float32), faces, AL.unalign_inv_ramp(feather, S), S)
        assert np.array_equal(out[0], photo), feather
    out = R.unalign_f32([photo], [0], fwd.astype(np.float32), 255.0 - faces, 2.0, S)
    assert not np.array_equal(out[0], photo) and np.array_equal(out[0][7:7 + S, 11:11 + S], 255 - photo[7:7 + S, 11:11 + S])


def test_row_order_matters_on_an_overlap():
    photos, boxes, coef, geom, faces = R.kernel_case()
    fwd = R.maps_f64(coef, geom, boxes[:, 0], R.hw_of(photos), S, S)[0].astype(np.float32)
    i, j = R.OVERLAPPING[0], R.OVERLAPPING[1]
    for feather in (0.0, 0.125):
        inv = AL.unalign_inv_ramp(feather, S)
        a, ca = R.unalign_f32(photos, boxes[[i, j], 0], fwd[[i, j]], faces[[i, j]], inv, S, return_cover=True)
        b = R.unalign_f32(photos, boxes[[j, i], 0], fwd[[j, i]], faces[[j, i]], inv, S)
        both = ca[0] & ca[1]
        assert both.sum() > 20 and (a[1][both] != b[1][both]).any(axis=1).mean() > 0.5
        assert np.array_equal(a[1][~both], b[1][~both])


def test_inv_ramp():
    assert AL.unalign_inv_ramp(0.0, 128) == 2.0 and AL.unalign_inv_ramp(0.125, 4) == 2.0           # 0.5 px: still a hard paste
    assert AL.unalign_inv_ramp(0.125, 128) == float(np.float32(1 / 16.0))
    assert AL.unalign_inv_ramp(0.5, 16) == 0.125 and AL.unalign_inv_ramp(0.3, 7) == float(np.float32(1 / (0.3 * 7)))


# ----------------------------------------------------------------------------------------------------------------------------
# refusals that need no device
# ----------------------------------------------------------------------------------------------------------------------------
def test_unalign_refusals():
    tpl = template()
    photos = [np.zeros((30, 40, 3), np.uint8), np.zeros((20, 25), np.uint8)]
    rows = np.array([(0, 2, 3, 20, 30), (1, 0, 0, 20, 25), (1, -5, -5, 10, 10)], dtype=np.int32)
    coef, geom = np.zeros((3, 3, 2), np.float32), np.ones((3, 4), np.float32)
    al = AL.Alignment(coef, geom, None, 'affine', 0.0, tpl, 64, rows)
    assert al.rows.dtype == np.int32 and al.rows.shape == (3, 5)
    ph, r, n, So, f = INF.plan_unalign(photos, (3, 64, 64, 3), al, 0.125)
    assert (n, So, f) == (3, 64, 0.125) and ph[1].shape == (20, 25, 3) and np.array_equal(r, rows)
    assert INF.plan_unalign(photos, (3, 64, 64, 4), al, 0.0)[4] == 0.0                       # wider pixels are fine
    with pytest.raises(NotImplementedError, match='tps map is not inverted'):
        INF.plan_unalign(photos, (3, 64, 64, 3), AL.Alignment(np.zeros((3, 8, 2)), geom, None, 'tps', 0.0, tpl, 64, rows), 0.125)
    with pytest.raises(ValueError, match='no box rows'):
        INF.plan_unalign(photos, (3, 64, 64, 3), AL.Alignment(coef, geom, None, 'affine', 0.0, tpl, 64), 0.125)
    for shape in ((2, 64, 64, 3), (4, 64, 64, 3)):                                           # a row count mismatch
        with pytest.raises(ValueError, match='aligned faces'):
            INF.plan_unalign(photos, shape, al, 0.125)
    for shape in ((3, 32, 32, 3), (3, 64, 64, 2), (3, 64, 64)):
        with pytest.raises(ValueError, match='aligned must be'):
            INF.plan_unalign(photos, shape, al, 0.125)
    with pytest.raises(ValueError, match='photos'):
        INF.plan_unalign(photos[:1], (3, 64, 64, 3), al, 0.125)                              # the rows name photo 1
    with pytest.raises(ValueError, match='list of u8 arrays'):
        INF.plan_unalign(np.zeros((2, 30, 40, 3), np.uint8), (3, 64, 64, 3), al, 0.125)
    for bad in (-0.1, 0.6, float('nan')):
        with pytest.raises(ValueError, match='feather'):
            INF.plan_unalign(photos, (3, 64, 64, 3), al, bad)
    # the grid hint: twice the largest box, at most the largest photo named
    assert INF.unalign_grid_pixels(ph, rows) == 2 * 20 * 25 and INF.unalign_grid_pixels(ph, rows[:1]) == 2 * 18 * 27 and INF.unalign_grid_pixels(ph, rows[2:]) == 2 * 15 * 15


def test_repose_template_refusals():
    tpl = template(10, 128)
    G.check_repose_template(tpl, 'similarity', 10, 128)
    G.check_repose_template(tpl, 'affine', 10, 128)
    with pytest.raises(NotImplementedError, match='tps map is not inverted'):
        G.check_repose_template(tpl, 'tps', 10, 128)
    with pytest.raises(ValueError, match='model'):
        G.check_repose_template(tpl, 'rigid', 10, 128)
    with pytest.raises(ValueError, match='template'):
        G.check_repose_template(tpl, 'affine', 12, 128)                                     # another K
    with pytest.raises(ValueError, match='template'):
        G.check_repose_template(tpl, 'affine', 10, 64)                                      # another S
    with pytest.raises(ValueError, match='LandmarkTemplate'):
        G.check_repose_template(np.zeros((10, 2)), 'affine', 10, 128)
    import inspect
    sig = inspect.signature(G.ImageGenerator.repose)
    assert list(sig.parameters)[-2:] == ['template', 'model']
    assert sig.parameters['template'].default is None and sig.parameters['model'].default == 'similarity'
    assert inspect.signature(INF.LandmarkDetector.unalign).parameters['feather'].default == 0.125


def test_generate_script_lists_the_template_arguments():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'generate.py'), '--help'], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-1500:]
    text = out.stdout.decode()
    assert '--template' in text and '--model' in text and 'similarity' in text and 'affine' in text and 'tps' not in text
