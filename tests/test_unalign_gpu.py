"""Unalign on the MI355X: imm_unalign_maps bit for bit against the f64 restatement of its arithmetic, imm_unalign_u8 bit for bit against
the f32 restatement of the pixel rule (tests/unalign_reference.py) and within the cap of the f64 one, its invariance under splitting a
call into launches, the identity case, LandmarkDetector.unalign against the restatement fed what align() returned, and
ImageGenerator.repose(template=) against the public composition align -> render -> restatement; repose without a template against
what it returned before, and the script."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compose_reference as CR                                               # noqa: E402
import guarded                                                               # noqa: E402
import unalign_reference as R                                                # noqa: E402
from alignment_reference import jittered_grid_template, smooth_photo          # noqa: E402
from dataset_fixtures import make_celeba_tree                                 # noqa: E402
from test_detector_gpu import _run_script, _write_config                      # noqa: E402
from test_detector_gpu import make_model as make_detector_model               # noqa: E402
from test_generator_gpu import make_model as make_generator_model             # noqa: E402

from imm_amd import alignment as AL                                           # noqa: E402
from imm_amd import generation as G                                           # noqa: E402
from imm_amd.inference import plan_buckets                                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SK = R.S_KERNEL
S = 128
FEATHERS = (0.0, 0.125, 0.5)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


def dev(ops, a):
    return ops.to_device_pinned(np.ascontiguousarray(a), DEV)


def run_maps(ops, coef, geom, boxes, hw, Si, So):
    """imm_unalign_maps in guarded buffers -> (fwd f32 [n, 6], bbox int32 [n, 4]) as host arrays."""
    n = len(boxes)
    guarded.reset()
    fwd = guarded.out((n, 6), torch.float32, DEV)
    bbox = guarded.out((n, 4), torch.int32, DEV)
    ops.unalign_maps(guarded.inp(torch.from_numpy(np.ascontiguousarray(coef)), DEV), guarded.inp(torch.from_numpy(np.ascontiguousarray(geom)), DEV),
                     guarded.inp(torch.from_numpy(np.ascontiguousarray(boxes)), DEV), dev(ops, hw), Si, So, fwd, bbox)
    torch.cuda.synchronize()
    guarded.check_guards()
    return fwd.cpu().numpy(), bbox.cpu().numpy()


def run_paste(ops, photos, boxes, fwd32, bbox, faces, feather, launches=None, So=SK, max_pixels=None):
    """imm_unalign_u8 over the packed photos in a guarded buffer, the rows issued as the given launches (lists of consecutive row indices,
    in order; default: one launch of all rows), the grid sized by max_pixels (default: the launch's largest bbox).  Returns (the whole buffer as a host array, the packed input buffer)."""
    buf, offs, hw = CR.pack(photos)
    guarded.reset()
    canvas = guarded.out(buf.shape, torch.uint8, DEV, fill=torch.from_numpy(buf))
    offs_d, hw_d = dev(ops, offs), dev(ops, hw)
    faces_d = guarded.inp(torch.from_numpy(faces), DEV)
    inv = AL.unalign_inv_ramp(feather, So)
    for part in ([list(range(len(boxes)))] if launches is None else launches):
        assert part == list(range(part[0], part[-1] + 1))                 # consecutive rows: their faces are a leading-dimension slice
        sl = slice(part[0], part[-1] + 1)
        area = int(max(1, ((bbox[sl, 2] - bbox[sl, 0]) * (bbox[sl, 3] - bbox[sl, 1])).max())) if max_pixels is None else max_pixels
        ops.unalign_u8(canvas, offs_d, hw_d, dev(ops, boxes[sl]), dev(ops, G.compose_links(boxes[sl])), dev(ops, fwd32[sl]), dev(ops, bbox[sl]),
                       inv, faces_d[sl], area)
    torch.cuda.synchronize()
    guarded.check_guards()
    return canvas.cpu().numpy(), buf


def same_bits(a, b):
    """f32 arrays equal bit for bit where finite, NaN where NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the map kernel
# ----------------------------------------------------------------------------------------------------------------------------
def test_unalign_maps_kernel(ops):
    photos, boxes, coef, geom, faces = R.kernel_case()
    hw = R.hw_of(photos)
    fwd, bbox = run_maps(ops, coef, geom, boxes, hw, SK, SK)
    want, want_bbox, _B, _t = R.maps_f64(coef, geom, boxes[:, 0], hw, SK, SK)
    assert same_bits(fwd, want.astype(np.float32)), 'imm_unalign_maps is not maps_f64 rounded to f32, bit for bit'
    bad = [R.SINGULAR_ROW] + list(R.BAD_IMAGE_ROWS)
    assert np.isnan(fwd[bad]).all() and not bbox[bad].any() and np.isfinite(np.delete(fwd, bad, axis=0)).all()
    assert np.array_equal(bbox, want_bbox)
    _out, covers = R.unalign_f32(photos, boxes[:, 0], fwd, faces, 2.0, SK, return_cover=True)
    for b, cov in enumerate(covers):
        if cov is not None:
            y0, x0, y1, x1 = bbox[b]
            cov = cov.copy()
            cov[y0:y1, x0:x1] = False
            assert not cov.any(), 'row %d covers a pixel outside its bbox' % b
    # more rows than one workgroup holds, S != So, maps of every orientation and a few degenerate ones
    rng = np.random.RandomState(11)
    n, Si, So = 150, 128, 96
    coef = rng.uniform(-1.5, 1.5, size=(n, 3, 2)).astype(np.float32)
    coef[::17, 2] = coef[::17, 1] * np.float32(2.0)                        # det == 0 exactly (a power-of-two multiple)
    geom = np.stack([rng.randint(-50, 300, n), rng.randint(-50, 300, n), rng.uniform(0.3, 3.0, n), rng.uniform(0.3, 3.0, n)], 1).astype(np.float32)
    boxes = np.zeros((n, 5), np.int32)
    boxes[:, 0] = rng.randint(-1, 4, n)                                    # -1 and 3 are no photos
    hw = np.array([[200, 300], [64, 64], [511, 7]], np.int32)
    fwd, bbox = run_maps(ops, coef, geom, boxes, hw, Si, So)
    want, want_bbox, _B, _t = R.maps_f64(coef, geom, boxes[:, 0], hw, Si, So)
    assert same_bits(fwd, want.astype(np.float32)) and np.array_equal(bbox, want_bbox)
    assert np.isnan(want[::17]).all() and np.isnan(want[(boxes[:, 0] < 0) | (boxes[:, 0] > 2)]).all() and np.isfinite(want).any()


# ----------------------------------------------------------------------------------------------------------------------------
# 2. the paste: parity, split invariance, identity
# ----------------------------------------------------------------------------------------------------------------------------
def case_maps(photos, boxes, coef, geom):
    fwd, bbox, B, t = R.maps_f64(coef, geom, boxes[:, 0], R.hw_of(photos), SK, SK)
    return fwd.astype(np.float32), bbox, B, t


@pytest.mark.parametrize('feather', FEATHERS)
@pytest.mark.parametrize('ld', [3, 12])
def test_unalign_kernel_parity(ops, ld, feather):
    photos, boxes, coef, geom, faces = R.kernel_case(ld=ld)
    assert (faces[..., :3] < 0).any() and (faces[..., :3] > 255).any() and (ld == 3 or np.isnan(faces[..., 3:]).all())
    fwd32, bbox, B, t = case_maps(photos, boxes, coef, geom)
    got, buf = run_paste(ops, photos, boxes, fwd32, bbox, faces, feather)
    inv = AL.unalign_inv_ramp(feather, SK)
    ref32, covers = R.unalign_f32(photos, boxes[:, 0], fwd32, faces, inv, SK, return_cover=True)
    ref64, covered, near = R.unalign_f64(photos, boxes[:, 0], B, t, faces, inv, SK)
    want, _o, _h = CR.pack(ref32)
    nbad = int((got != want).sum())
    print('\nUNALIGN KERNEL ld=%d feather=%g: %d of %d bytes differ from the f32 restatement' % (ld, feather, nbad, got.size))
    assert np.array_equal(got, want), 'the kernel is not the f32 restatement bit for bit'
    n_diff, worst, n_near, n_cov = R.within_cap(CR.unpack(got, photos), ref64, covered, near)
    print('UNALIGN KERNEL vs f64: %d of %d covered pixels differ (max %d), %d in the border band' % (n_diff, n_cov, worst, n_near))
    # every byte no row covers - other pixels, the photo without a row, the padding between photos - is the input's
    masks = [np.zeros(p.shape[:2], dtype=bool) for p in photos]
    for b, cov in enumerate(covers):
        if cov is not None:
            masks[boxes[b, 0]] |= cov
    inside, _o, _h = CR.pack([np.repeat(m[:, :, None], 3, axis=2).astype(np.uint8) for m in masks])
    inside = inside == 1                                                  # (the padding of that buffer holds 0xA5)
    assert inside.sum() == 3 * sum(int(m.sum()) for m in masks) and not masks[3].any()
    assert np.array_equal(got[~inside], buf[~inside])
    assert (got[inside] != buf[inside]).mean() > 0.5


def test_unalign_split_invariance(ops):
    photos, boxes, coef, geom, faces = R.kernel_case(ld=12)
    fwd32, bbox, _B, _t = case_maps(photos, boxes, coef, geom)
    n = len(boxes)
    for feather in (0.0, 0.125):
        one, _ = run_paste(ops, photos, boxes, fwd32, bbox, faces, feather)
        two, _ = run_paste(ops, photos, boxes, fwd32, bbox, faces, feather, [list(range(0, 4)), list(range(4, n))])
        each, _ = run_paste(ops, photos, boxes, fwd32, bbox, faces, feather, [[i] for i in range(n)])
        assert np.array_equal(one, two) and np.array_equal(one, each), feather
    # the two-launch split parts the three mutually overlapping rows
    assert sum(i < 4 for i in R.OVERLAPPING) == 2


def test_unalign_one_block_per_row(ops):
    """The grid-size argument set to 1: ONE block of 256 threads per row carries every box through the grid-stride loop, and the bytes
    are those of a grid as large as the largest box."""
    photos, boxes, coef, geom, faces = R.kernel_case(ld=12)
    fwd32, bbox, _B, _t = case_maps(photos, boxes, coef, geom)
    assert ((bbox[:, 2] - bbox[:, 0]) * (bbox[:, 3] - bbox[:, 1])).max() > 2 * 256
    for feather in (0.0, 0.125):
        full, _ = run_paste(ops, photos, boxes, fwd32, bbox, faces, feather)
        one, _ = run_paste(ops, photos, boxes, fwd32, bbox, faces, feather, max_pixels=1)
        assert np.array_equal(one, full), feather


def test_unalign_identity(ops):
    rng = np.random.RandomState(1)
    photos = [rng.randint(0, 256, size=(31, 45, 3)).astype(np.uint8), rng.randint(0, 256, size=(16, 16, 3)).astype(np.uint8)]
    at = [(7, 11), (0, 0)]
    pairs = [R.coefficients_of(np.eye(2), np.array(p, dtype=np.float64), SK, SK) for p in at]
    coef, geom = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    boxes = np.array([(0, 0, 0, 1, 1), (1, 0, 0, 1, 1)], dtype=np.int32)
    fwd, bbox = run_maps(ops, coef, geom, boxes, R.hw_of(photos), SK, SK)
    assert np.array_equal(fwd, np.array([[1, 0, -7, 0, 1, -11], [1, 0, 0, 0, 1, 0]], np.float32))
    faces = np.stack([R.float_crop(photos[i], y, x, SK) for i, (y, x) in enumerate(at)])
    for feather in (0.0, 0.125, 0.25, 0.5):
        got, buf = run_paste(ops, photos, boxes, fwd, bbox, faces, feather)
        assert np.array_equal(got, buf), feather
    # and the paste is no no-op: other faces change the quad
    got, buf = run_paste(ops, photos, boxes, fwd, bbox, 255.0 - faces, 0.25)
    assert not np.array_equal(got, buf)


def test_unalign_wrapper_refusals(ops):
    z = lambda *sh, **kw: torch.zeros(*sh, device=DEV, **kw)
    photos, offs, hw = z(64, dtype=torch.uint8), z(1, dtype=torch.int64), z(1, 2, dtype=torch.int32)
    boxes, links, fwd, bbox, faces = z(2, 5, dtype=torch.int32), z(2, 2, dtype=torch.int32), z(2, 6), z(2, 4, dtype=torch.int32), z(2, 16, 16, 3)
    with pytest.raises(ValueError, match='links'):
        ops.unalign_u8(photos, offs, hw, boxes, links[:1], fwd, bbox, 2.0, faces, 16)
    with pytest.raises(ValueError, match='fwd'):
        ops.unalign_u8(photos, offs, hw, boxes, links, fwd.double(), bbox, 2.0, faces, 16)
    with pytest.raises(ValueError, match='bbox'):
        ops.unalign_u8(photos, offs, hw, boxes, links, fwd, bbox.long(), 2.0, faces, 16)
    with pytest.raises(ValueError, match='faces'):
        ops.unalign_u8(photos, offs, hw, boxes, links, fwd, bbox, 2.0, z(2, 16, 16, 2), 16)
    with pytest.raises(ValueError, match='photos'):
        ops.unalign_u8(photos.float(), offs, hw, boxes, links, fwd, bbox, 2.0, faces, 16)
    with pytest.raises(ValueError, match='coef'):
        ops.unalign_maps(z(2, 13, 2), z(2, 4), boxes, hw, 128, 128, fwd, bbox)            # a tps coefficient block
    with pytest.raises(ValueError, match='geom'):
        ops.unalign_maps(z(2, 3, 2), z(2, 3), boxes, hw, 128, 128, fwd, bbox)
    with pytest.raises(ValueError, match='bbox'):
        ops.unalign_maps(z(2, 3, 2), z(2, 4), boxes, hw, 128, 128, fwd, bbox[:1])


# ----------------------------------------------------------------------------------------------------------------------------
# 3. LandmarkDetector.unalign
# ----------------------------------------------------------------------------------------------------------------------------
def own_template(mu, deg=35.0, scale=1.25):
    """A template from the model's own landmarks mu [n, K, 2]: their mean shape, turned and enlarged about its centroid, so that the
    alignment maps rotate and scale by about that much (an untrained model's landmarks sit in a small cloud; a template spread over
    the whole frame would shrink every aligned face to a few photo pixels)."""
    m = mu.double().cpu().numpy().mean(axis=0)
    th = np.deg2rad(deg)
    rot = scale * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    return AL.LandmarkTemplate((m - m.mean(axis=0)) @ rot.T + m.mean(axis=0), S)


def restate(ims, al, aligned, feather):
    """unalign_f32 fed what align() returned."""
    rows = al.rows
    fwd = R.maps_f64(al.coef.cpu().numpy(), al.geom.cpu().numpy(), rows[:, 0], R.hw_of(ims), S, al.out_size)[0].astype(np.float32)
    return R.unalign_f32(ims, rows[:, 0], fwd, aligned.cpu().numpy(), AL.unalign_inv_ramp(feather, al.out_size), al.out_size,
                         return_cover=True)


SURFACE_SIZES = [(96, 90), (80, 96), (77, 61), (96, 96), (64, 95), (90, 70)]
# one row per photo and a second one on photo 1 that overlaps the first: 7 rows, two buckets at max_batch = 4
SURFACE_BOXES = [(0, 4, 3, 92, 86), (1, 0, 6, 70, 90), (2, -8, -5, 70, 58), (3, 10, 10, 96, 96), (4, 2, 20, 60, 88), (1, 20, 0, 80, 70),
                 (5, 5, 5, 100, 75)]


@pytest.mark.parametrize('kind', ['similarity', 'affine'])
def test_detector_unalign_against_the_restatement(ops, kind):
    from imm_amd.inference import LandmarkDetector
    cfg, model, eng, P, St = make_detector_model(10, S, 2)
    det = model.landmark_detector(S, max_batch=4)
    ims = [smooth_photo(h, w, 60 + i) for i, (h, w) in enumerate(SURFACE_SIZES)]
    assert len(plan_buckets(len(SURFACE_BOXES), 4)) == 2
    tpl = own_template(det.landmarks(ims, SURFACE_BOXES))
    So = 64 if kind == 'affine' else S
    aligned, al = det.align(ims, tpl, SURFACE_BOXES, kind, out_size=So, return_transform=True)
    assert al.rows.shape == (7, 5) and al.rows.dtype == np.int32 and al.rows[:, 0].tolist() == [b[0] for b in SURFACE_BOXES]
    n_cov = 0
    for feather in (0.125, 0.0):
        out = det.unalign(ims, aligned, al, feather)
        torch.cuda.synchronize()
        want, covers = restate(ims, al, aligned, feather)
        assert len(out) == len(ims)
        for o, w, im in zip(out, want, ims):
            assert o.dtype == torch.uint8 and o.device.type == 'cuda' and tuple(o.shape) == im.shape
            assert torch.equal(o.cpu(), torch.from_numpy(w)), 'unalign != the restatement fed align()\'s coef and geom (%s, feather %g)' % (
                kind, feather)
        n_cov = sum(int(c.sum()) for c in covers)
        changed = sum(int((o.cpu().numpy() != im).any(axis=2).sum()) for o, im in zip(out, ims))
        print('\nUNALIGN() %s So=%d feather=%g: %d covered pixels, %d changed' % (kind, So, feather, n_cov, changed))
    assert n_cov > 0
    # the star form of the issue, host faces, and faces of a wider pixel stride read in place
    star = det.unalign(ims, *det.align(ims, tpl, SURFACE_BOXES, kind, out_size=So, return_transform=True))
    wide = torch.full((7, So, So, 5), float('nan'), device=DEV)
    wide[..., :3] = aligned
    for other in (star, det.unalign(ims, aligned.cpu().numpy(), al), det.unalign(ims, wide, al)):
        assert all(torch.equal(x, torch.from_numpy(w)) for x, w in zip([o.cpu() for o in other], restate(ims, al, aligned, 0.125)[0]))
    # captured graphs and plain launches give the same bytes
    plain = LandmarkDetector(model, S, max_batch=4, use_graph=False)
    aligned2, al2 = plain.align(ims, tpl, SURFACE_BOXES, kind, out_size=So, return_transform=True)
    assert torch.equal(aligned2, aligned) and torch.equal(al2.coef, al.coef)
    assert all(torch.equal(x, y) for x, y in zip(plain.unalign(ims, aligned2, al2), star))
    # the photos handed in are not written
    assert all(np.array_equal(im, smooth_photo(h, w, 60 + i)) for i, (im, (h, w)) in enumerate(zip(ims, SURFACE_SIZES)))


def test_detector_unalign_refusals(ops):
    cfg, model, eng, P, St = make_detector_model(10, S, 2)
    det = model.landmark_detector(S, max_batch=4)
    ims = [smooth_photo(h, w, 60 + i) for i, (h, w) in enumerate(SURFACE_SIZES[:2])]
    tpl = AL.LandmarkTemplate(jittered_grid_template(10, 8), S)
    aligned, al = det.align(ims, tpl, model='tps', out_size=32, return_transform=True)
    with pytest.raises(NotImplementedError, match='tps map is not inverted'):
        det.unalign(ims, aligned, al)
    aligned, al = det.align(ims, tpl, out_size=32, return_transform=True)
    with pytest.raises(ValueError, match='aligned faces'):
        det.unalign(ims, aligned[:1], al)
    with pytest.raises(ValueError, match='photos'):
        det.unalign(ims[:1], aligned, al)
    with pytest.raises(ValueError, match='feather'):
        det.unalign(ims, aligned, al, 0.75)
    # a tensor batch has no photos to paste into
    crops = torch.zeros(2, S, S, 3)
    _img, al_t = det.align(crops, tpl, out_size=32, return_transform=True)
    assert al_t.rows is None
    with pytest.raises(ValueError, match='no box rows'):
        det.unalign(ims, aligned, al_t)


# ----------------------------------------------------------------------------------------------------------------------------
# 4. ImageGenerator.repose(template=)
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def m128(ops):
    return make_generator_model(10, S, 4)


@pytest.fixture(scope='module')
def scene():
    from test_compose_gpu import FACE_BOXES, PHOTO_SIZES
    from imm_amd import keypoints as KP
    ims = [smooth_photo(h, w, 20 + i) for i, (h, w) in enumerate(PHOTO_SIZES)]
    rows = KP.check_boxes(FACE_BOXES, len(ims))
    lm = torch.from_numpy(np.random.RandomState(4).uniform(-0.7, 0.7, size=(5, 10, 2)).astype(np.float32))
    return ims, rows, lm, FACE_BOXES


@pytest.mark.parametrize('kind', ['similarity', 'affine'])
def test_repose_with_a_template_against_the_public_composition(m128, scene, kind):
    cfg, model, eng, P, St = m128
    ims, rows, lm, face_boxes = scene
    gen = model.image_generator(S, max_batch=4)
    buckets = plan_buckets(len(rows), 4)
    assert len(buckets) == 2
    tpl = own_template(gen.detector.landmarks(ims, face_boxes))
    for feather in (0.125, 0.0):
        aligned, al = gen.detector.align(ims, tpl, face_boxes, kind, return_transform=True)
        faces_pub = torch.cat([gen.render(aligned[s:s + c], lm[s:s + c]) for s, c, _b in buckets])
        torch.cuda.synchronize()
        want, covers = restate(ims, al, faces_pub, feather)
        out, faces, lm_used = gen.repose(ims, lm, face_boxes, feather=feather, return_faces=True, template=tpl, model=kind)
        torch.cuda.synchronize()
        assert len(out) == 3 and torch.equal(lm_used.cpu(), lm) and torch.equal(faces, faces_pub)
        for o, w, im in zip(out, want, ims):
            assert o.dtype == torch.uint8 and o.device.type == 'cuda' and tuple(o.shape) == im.shape
            assert torch.equal(o.cpu(), torch.from_numpy(w)), 'repose(template=) != align -> render -> restatement (%s, feather %g)' % (
                kind, feather)
        n_cov = sum(int(c.sum()) for c in covers)
        print('\nREPOSE(template) %s feather=%g: %d covered pixels' % (kind, feather, n_cov))
        assert n_cov > 0
        # a second call gives the same bytes, and leaves the first call's result alone
        before = [o.clone() for o in out]
        again = gen.repose(ims, lm, face_boxes, feather=feather, template=tpl, model=kind)
        assert all(torch.equal(x, y) for x, y in zip(before, again)) and all(torch.equal(x, y) for x, y in zip(before, out))
    # pose photos: landmarks in the aligned frame
    pose_photos = [smooth_photo(150, 140, 31)]
    mu = gen.detector.detect(gen.detector.align(pose_photos, tpl, None, kind))
    a = gen.repose(ims, pose_photos, face_boxes, template=tpl, model=kind)
    b = gen.repose(ims, mu, face_boxes, template=tpl, model=kind)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(np.array_equal(im, smooth_photo(*im.shape[:2], 20 + i)) for i, im in enumerate(ims))


def test_repose_refusals_and_the_path_without_a_template(m128, scene):
    from test_compose_gpu import host_compose
    cfg, model, eng, P, St = m128
    ims, rows, lm, face_boxes = scene
    gen = model.image_generator(S, max_batch=4)
    tpl = AL.LandmarkTemplate(jittered_grid_template(10, 8), S)
    with pytest.raises(NotImplementedError, match='tps map is not inverted'):
        gen.repose(ims, lm, face_boxes, template=tpl, model='tps')
    with pytest.raises(ValueError):
        gen.repose(ims, lm, face_boxes, template=AL.LandmarkTemplate(jittered_grid_template(11, 8), S))
    with pytest.raises(ValueError, match='feather'):
        gen.repose(ims, lm, face_boxes, feather=0.7, template=tpl)
    # without a template: exactly the composition of before (host crops -> render -> compose_reference), also after a template call
    gen.repose(ims, lm, face_boxes, template=tpl)
    for feather in (0.125, 0.0):
        want, faces_host = host_compose(gen, ims, rows, lm, feather)
        out, faces, _lm = gen.repose(ims, lm, face_boxes, feather=feather, return_faces=True)
        assert torch.equal(faces, faces_host)
        assert all(torch.equal(o.cpu(), torch.from_numpy(w)) for o, w in zip(out, want))
        assert all(torch.equal(x, y) for x, y in zip(out, gen.repose(ims, lm, face_boxes, feather=feather, template=None, model='affine')))


def test_generate_script_reposes_photos_through_a_template(m128, tmp_path, capsys):
    from PIL import Image
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
    lm = np.random.RandomState(2).uniform(-0.6, 0.6, size=(4, 10, 2)).astype(np.float32)
    np.savez(str(tmp_path / 'lm.npz'), landmarks=lm)
    tplp = str(tmp_path / 'template.npz')
    AL.LandmarkTemplate(jittered_grid_template(10, 8), S).save(tplp)
    script = os.path.join(ROOT, 'scripts', 'generate.py')
    common = ['--configs', conf, '--checkpoint', ckpt, '--appearance-dir', imdir, '--boxes', boxes, '--batch-size', '4', '--template', tplp]
    pose_boxes = str(tmp_path / 'poses.csv')
    with open(pose_boxes, 'w') as f:
        f.write(''.join('%s,%d,%d,%d,%d\n' % (names[k], 10, 10, 200, 160) for k in (1, 3, 4, 1)))
    for k, extra in enumerate((['--landmarks', str(tmp_path / 'lm.npz')],
                               ['--pose-dir', imdir, '--pose-boxes', pose_boxes, '--model', 'affine', '--feather', '0'])):
        out_dir = str(tmp_path / ('reposed%d' % k))
        _run_script(script, common + extra + ['--out-dir', out_dir])
        assert '4 faces re-posed in 6 photos' in capsys.readouterr().out
        assert sorted(os.listdir(out_dir)) == [n.replace('.jpg', '.png') for n in names]
        for n in names:
            png = np.asarray(Image.open(os.path.join(out_dir, n.replace('.jpg', '.png'))))
            assert png.shape == pixels[n].shape and png.dtype == np.uint8
            if n not in (names[0], names[2], names[5]):
                assert np.array_equal(png, pixels[n]), n                     # a photo without a face row comes back as it was
    with pytest.raises(SystemExit):
        _run_script(script, common + ['--landmarks', str(tmp_path / 'lm.npz'), '--model', 'tps', '--out-dir', str(tmp_path / 'no')])
