"""Compose on the MI355X: imm_compose_u8 bit for bit against the f32 restatement of its pixel rule (tests/compose_reference.py) and
within the cap of the f64 one, its invariance under splitting a call into launches, the identity case, and ImageGenerator.repose
against a composition made on the host from host crops, render() in the same bucket and the restatement; pose photos, boxes= of the
other calls, repeatability, the program's shape and the script."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import image_oracle as IO

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compose_reference as R                                                # noqa: E402
import guarded                                                               # noqa: E402
from alignment_reference import smooth_photo                                  # noqa: E402
from dataset_fixtures import make_celeba_tree                                 # noqa: E402
from test_detector_gpu import _run_script, _write_config                      # noqa: E402
from test_generator_gpu import make_model                                     # noqa: E402

from imm_amd import generation as G                                           # noqa: E402
from imm_amd.inference import plan_buckets                                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SK = R.S_KERNEL
S = 128


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


@pytest.fixture(scope='module')
def m128(ops):
    return make_model(10, S, 4)


def dev(ops, a):
    return ops.to_device_pinned(np.ascontiguousarray(a), DEV)


def run_compose(ops, photos, rows, faces, feather, launches=None, max_pixels=None):
    """imm_compose_u8 over the packed photos in a guarded buffer, the rows issued as the given launches (lists of row indices, in
    order; default: one launch of all rows), the grid sized by max_pixels (default: the launch's largest box).  Returns (the whole buffer as a host array, the packed input buffer)."""
    buf, offs, hw = R.pack(photos)
    guarded.reset()
    canvas = guarded.out(buf.shape, torch.uint8, DEV, fill=torch.from_numpy(buf))
    offs_d, hw_d = dev(ops, offs), dev(ops, hw)
    faces_d = guarded.inp(torch.from_numpy(faces), DEV)
    for part in ([list(range(len(rows)))] if launches is None else launches):
        sub = rows[part]
        area = int(((sub[:, 3] - sub[:, 1]) * (sub[:, 4] - sub[:, 2])).max()) if max_pixels is None else max_pixels
        assert part == list(range(part[0], part[-1] + 1))                 # consecutive rows: their faces are a leading-dimension slice
        ops.compose_u8(canvas, offs_d, hw_d, dev(ops, sub), dev(ops, G.compose_links(sub)), dev(ops, G.compose_inv_ramp(sub, feather)),
                       faces_d[part[0]:part[-1] + 1], area)
    torch.cuda.synchronize()
    guarded.check_guards()
    return canvas.cpu().numpy(), buf


# ----------------------------------------------------------------------------------------------------------------------------
# 1. parity, 2. split invariance, 3. identity
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('feather', [0.0, 0.125, 0.5])
@pytest.mark.parametrize('ld', [3, 4])
def test_compose_kernel_parity(ops, ld, feather):
    photos, rows, faces = R.kernel_case(ld=ld)
    assert (faces[..., :3] < 0).any() and (faces[..., :3] > 255).any()
    got, buf = run_compose(ops, photos, rows, faces, feather)
    ramp = G.compose_inv_ramp(rows, feather)
    ref32 = R.compose_f32(photos, rows, faces, ramp, SK)
    ref64 = R.compose_f64(photos, rows, faces, ramp, SK)
    want, _o, _h = R.pack(ref32)
    nbad = int((got != want).sum())
    print('\nCOMPOSE KERNEL ld=%d feather=%g: %d of %d bytes differ from the f32 restatement' % (ld, feather, nbad, got.size))
    assert np.array_equal(got, want), 'the kernel is not the f32 restatement bit for bit'
    masks = R.box_mask(photos, rows)
    n_box = 3 * sum(int(m.sum()) for m in masks)
    diff = np.concatenate([np.abs(a.astype(np.int64) - b.astype(np.int64)).reshape(-1) for a, b in zip(R.unpack(got, photos), ref64)])
    print('COMPOSE KERNEL vs f64: %d of %d box bytes differ (max %d)' % (int((diff > 0).sum()), n_box, int(diff.max())))
    assert diff.max() <= 1 and (diff > 0).sum() <= 0.005 * n_box
    # every byte outside every box - other pixels, the photo without a box, the padding between photos - is the input's
    inside, _o, _h = R.pack([np.repeat(m[:, :, None], 3, axis=2).astype(np.uint8) for m in masks])
    inside = inside == 1                                                  # (the padding of that buffer holds 0xA5)
    assert inside.sum() == n_box
    assert np.array_equal(got[~inside], buf[~inside])
    assert (got[inside] != buf[inside]).mean() > 0.5


def test_compose_split_invariance(ops):
    photos, rows, faces = R.kernel_case(ld=4)
    n = len(rows)
    for feather in (0.0, 0.125):
        one, _ = run_compose(ops, photos, rows, faces, feather)
        pairs, _ = run_compose(ops, photos, rows, faces, feather, [list(range(i, min(i + 2, n))) for i in range(0, n, 2)])
        # the three mutually overlapping rows 2, 6, 10 in three launches
        apart, _ = run_compose(ops, photos, rows, faces, feather, [list(range(0, 5)), list(range(5, 9)), list(range(9, n))])
        assert np.array_equal(one, pairs) and np.array_equal(one, apart), feather
    assert all(sum(i in part for i in R.OVERLAPPING) == 1 for part in (range(0, 5), range(5, 9), range(9, n)))


def test_compose_one_block_per_row(ops):
    """The grid-size argument set to 1: ONE block of 256 threads per row carries every box through the grid-stride loop, and the bytes
    are those of a grid as large as the largest box."""
    photos, rows, faces = R.kernel_case(ld=4)
    assert ((rows[:, 3] - rows[:, 1]) * (rows[:, 4] - rows[:, 2])).max() > 2 * 256
    for feather in (0.0, 0.125):
        full, _ = run_compose(ops, photos, rows, faces, feather)
        one, _ = run_compose(ops, photos, rows, faces, feather, max_pixels=1)
        assert np.array_equal(one, full), feather


def test_compose_identity(ops):
    rng = np.random.RandomState(1)
    photos = [rng.randint(0, 256, size=(31, 45, 3)).astype(np.uint8), rng.randint(0, 256, size=(16, 16, 3)).astype(np.uint8)]
    rows = np.array([(0, 7, 11, 7 + SK, 11 + SK), (1, 0, 0, SK, SK)], dtype=np.int32)
    faces = np.stack([R.float_crop(photos[i], rows[i, 1:], SK) for i in range(2)])
    for feather in (0.0, 0.25):
        got, buf = run_compose(ops, photos, rows, faces, feather)
        assert np.array_equal(got, buf), feather
    # and the paste is no no-op: other faces change the box
    got, buf = run_compose(ops, photos, rows, 255.0 - faces, 0.25)
    assert not np.array_equal(got, buf)


def test_compose_wrapper_refusals(ops):
    z = lambda *sh, **kw: torch.zeros(*sh, device=DEV, **kw)
    photos, offs, hw = z(64, dtype=torch.uint8), z(1, dtype=torch.int64), z(1, 2, dtype=torch.int32)
    boxes, links, ramp, faces = z(2, 5, dtype=torch.int32), z(2, 2, dtype=torch.int32), z(2, 2), z(2, 16, 16, 3)
    with pytest.raises(ValueError, match='links'):
        ops.compose_u8(photos, offs, hw, boxes, links[:1], ramp, faces, 16)
    with pytest.raises(ValueError, match='inv_ramp'):
        ops.compose_u8(photos, offs, hw, boxes, links, ramp.double(), faces, 16)
    with pytest.raises(ValueError, match='faces'):
        ops.compose_u8(photos, offs, hw, boxes, links, ramp, z(2, 16, 16, 2), 16)
    with pytest.raises(ValueError, match='photos'):
        ops.compose_u8(photos.float(), offs, hw, boxes, links, ramp, faces, 16)


# ----------------------------------------------------------------------------------------------------------------------------
# 4. .. 8. ImageGenerator.repose
# ----------------------------------------------------------------------------------------------------------------------------
PHOTO_SIZES = [(200, 170), (190, 176), (208, 165)]
# rows 1 and 3 overlap on photo 1 (given with a row of another photo between them); row 4 leaves photo 2 at the bottom right
FACE_BOXES = [(0, 20, 15, 180, 150), (1, 10, 8, 130, 120), (2, 5, 30, 100, 140), (1, 70, 60, 185, 170), (2, 120, 90, 240, 200)]


def crop_to_box(image, box):
    from imm_amd.datasets.impair_dataset import ImagePairDataset
    return ImagePairDataset._crop_to_box(None, image, box, pad=True)


def host_crops(ims, rows):
    return torch.from_numpy(np.stack([IO.resize_bilinear(crop_to_box(ims[i], (y0, x0, y1, x1)), S, S) for i, y0, x0, y1, x1 in rows]))


def host_compose(gen, ims, rows, lm, feather):
    """The composition made on the host: host crops, render() bucket by bucket as repose() splits the rows, the f32 restatement."""
    crops = host_crops(ims, rows)
    faces = torch.cat([gen.render(crops[s:s + c], lm[s:s + c]) for s, c, _b in plan_buckets(len(rows), gen.max_batch)])
    torch.cuda.synchronize()
    return R.compose_f32(ims, rows, faces.cpu().numpy(), G.compose_inv_ramp(rows, feather), S), faces


@pytest.fixture(scope='module')
def scene():
    from imm_amd import keypoints as KP
    ims = [smooth_photo(h, w, 20 + i) for i, (h, w) in enumerate(PHOTO_SIZES)]
    rows = KP.check_boxes(FACE_BOXES, len(ims))
    lm = torch.from_numpy(np.random.RandomState(4).uniform(-0.7, 0.7, size=(5, 10, 2)).astype(np.float32))
    return ims, rows, lm


@pytest.mark.parametrize('max_batch', [8, 2])
def test_repose_against_the_host_composition(m128, scene, max_batch):
    cfg, model, eng, P, St = m128
    ims, rows, lm = scene
    gen = model.image_generator(S, max_batch=max_batch)
    assert len(plan_buckets(5, max_batch)) == (1 if max_batch == 8 else 3)
    for feather in (0.125, 0.0):
        want, faces_host = host_compose(gen, ims, rows, lm, feather)
        out, faces, lm_used = gen.repose(ims, lm, FACE_BOXES, feather=feather, return_faces=True)
        torch.cuda.synchronize()
        assert len(out) == 3 and torch.equal(lm_used.cpu(), lm)
        for o, w, im in zip(out, want, ims):
            assert o.dtype == torch.uint8 and o.device.type == 'cuda' and tuple(o.shape) == im.shape
            assert torch.equal(o.cpu(), torch.from_numpy(w)), 'repose != host crops -> render -> restatement (feather %g)' % feather
        assert torch.equal(faces, faces_host)
        masks = R.box_mask(ims, rows)
        for o, im, m in zip(out, ims, masks):
            o = o.cpu().numpy()
            assert np.array_equal(o[~m], im[~m]) and (o[m] != im[m]).mean() > 0.5
    # the second row of the overlapping pair was cut from the ORIGINAL pixels, not from the photo with the first face in it
    # (faces[3] above is render() of the crop of ims[1]; the crop of the same box from the pasted photo is another image)
    pasted = R.compose_f32(ims, rows[1:2], faces_host[1:2].cpu().numpy(), G.compose_inv_ramp(rows[1:2], 0.0), S)
    assert torch.equal(faces[3], faces_host[3])
    assert not torch.equal(host_crops(pasted, rows[3:4]), host_crops(ims, rows[3:4]))


def test_repose_pose_photos_and_broadcast(m128, scene):
    cfg, model, eng, P, St = m128
    ims, rows, lm = scene
    gen = model.image_generator(S, max_batch=8)
    pose_photos = [smooth_photo(150, 140, 31), smooth_photo(128, 128, 32)]
    pose_boxes = [(0, 10, 10, 140, 130), (1, 0, 0, 128, 128), (0, -10, 20, 100, 120), (1, 20, 20, 110, 100), (0, 0, 0, 150, 140)]
    mu = gen.detector.landmarks(pose_photos, pose_boxes)
    a = gen.repose(ims, pose_photos, FACE_BOXES, pose_boxes)
    b = gen.repose(ims, mu, FACE_BOXES)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # one pose for every row: a single pose photo, a single landmark set, and that set repeated
    one = gen.repose(ims, pose_photos[:1], FACE_BOXES)
    mu1 = gen.detector.landmarks(pose_photos[:1])
    for other in (gen.repose(ims, mu1, FACE_BOXES), gen.repose(ims, mu1.expand(5, 10, 2).contiguous(), FACE_BOXES)):
        assert all(torch.equal(x, y) for x, y in zip(one, other))
    assert not all(torch.equal(x, y) for x, y in zip(one, a))
    # without boxes: one whole-photo box per photo
    whole = gen.repose(ims, mu[:3])
    boxed = gen.repose(ims, mu[:3], [(0, 0) + im.shape[:2] for im in ims])
    assert all(torch.equal(x, y) for x, y in zip(whole, boxed))
    with pytest.raises(ValueError):
        gen.repose(ims, mu[:2], FACE_BOXES)


def test_return_faces_and_boxes_of_the_other_calls(m128, scene):
    cfg, model, eng, P, St = m128
    ims, rows, lm = scene
    gen = model.image_generator(S, max_batch=8)
    crops = host_crops(ims, rows)
    _out, faces, _lm = gen.repose(ims, lm, FACE_BOXES, return_faces=True)
    rendered = gen.render(ims, lm, boxes=FACE_BOXES)
    assert faces.shape == (5, S, S, 3) and torch.equal(faces, rendered) and torch.equal(rendered, gen.render(crops, lm))
    pose_photos = [smooth_photo(150, 140, 31), smooth_photo(128, 128, 32)]
    pose_boxes = [(0, 10, 10, 140, 130), (1, 0, 0, 128, 128), (0, -10, 20, 100, 120), (1, 20, 20, 110, 100), (0, 0, 0, 150, 140)]
    from imm_amd import keypoints as KP
    pose_crops = host_crops(pose_photos, KP.check_boxes(pose_boxes, 2))
    assert torch.equal(gen.reconstruct(ims, pose_photos, boxes=FACE_BOXES, pose_boxes=pose_boxes), gen.reconstruct(crops, pose_crops))
    # transfer: 5 x 5 pairs run in buckets of 8 on both sides
    assert torch.equal(gen.transfer(ims, pose_photos, boxes=FACE_BOXES, pose_boxes=pose_boxes), gen.transfer(crops, pose_crops))
    with pytest.raises(ValueError, match='boxes need the images as a list of u8 arrays'):
        gen.render(crops, lm, boxes=FACE_BOXES)
    with pytest.raises(ValueError):
        gen.reconstruct(ims, pose_photos, boxes=FACE_BOXES, pose_boxes=pose_boxes[:4])


def test_repose_repeatability_and_graph_mode(m128, scene):
    from imm_amd.generation import ImageGenerator
    cfg, model, eng, P, St = m128
    ims, rows, lm = scene
    gen = model.image_generator(S, max_batch=4)                                # two buckets: 4 rows and 1
    a = gen.repose(ims, lm, FACE_BOXES)
    before = [x.clone() for x in a]
    b = gen.repose(ims, lm, FACE_BOXES)
    assert all(torch.equal(x, y) for x, y in zip(before, b))
    assert all(torch.equal(x, y) for x, y in zip(before, a)), 'a later call changed an earlier result'
    plain = ImageGenerator(model, S, max_batch=4, use_graph=False)
    assert all(torch.equal(x, y) for x, y in zip(before, plain.repose(ims, lm, FACE_BOXES)))
    # the photos handed in are not written
    assert all(np.array_equal(im, smooth_photo(h, w, 20 + i)) for i, (im, (h, w)) in enumerate(zip(ims, PHOTO_SIZES)))


def test_repose_program_shape(m128):
    cfg, model, eng, P, St = m128
    gen = model.image_generator(S, max_batch=8)
    app, ren = gen.program('appearance', 8), gen.program('render', 8)
    prog = gen.program('compose', 8)
    assert [(l.tag, l.family) for l in prog[:-1]] == [(l.tag, l.family) for l in app + ren]
    assert len(prog) == len(app) + len(ren) + 1
    assert (prog[-1].tag, prog[-1].family) == ('compose', 'compose') and [l.tag for l in prog].count('compose') == 1
    with pytest.raises(ValueError):
        gen.program('paste', 8)
    # and that is what a call issues: per bucket one appearance run, one render run, one compose launch
    calls = []
    run0, compose0 = gen._run, G.ops.compose_u8
    gen._run = lambda stage, b: (calls.append(stage), run0(stage, b))
    G.ops.compose_u8 = lambda *a, **k: (calls.append('compose'), compose0(*a, **k))
    try:
        gen.repose([smooth_photo(90, 80, 1)] * 3, torch.zeros(1, 10, 2))
    finally:
        del gen._run
        G.ops.compose_u8 = compose0
    assert calls == ['appearance', 'render', 'compose']


# ----------------------------------------------------------------------------------------------------------------------------
# 9. the script
# ----------------------------------------------------------------------------------------------------------------------------
def test_generate_script_reposes_photos(m128, tmp_path, capsys):
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
    out_dir = str(tmp_path / 'reposed')
    _run_script(os.path.join(ROOT, 'scripts', 'generate.py'), ['--configs', conf, '--checkpoint', ckpt, '--appearance-dir', imdir, '--boxes', boxes,
                                                               '--landmarks', str(tmp_path / 'lm.npz'), '--out-dir', out_dir, '--batch-size', '4'])
    assert '4 faces re-posed in 6 photos' in capsys.readouterr().out
    assert sorted(os.listdir(out_dir)) == [n.replace('.jpg', '.png') for n in names]
    for i, n in enumerate(names):
        png = np.asarray(Image.open(os.path.join(out_dir, n.replace('.jpg', '.png'))))
        src = pixels[n]
        assert png.shape == src.shape and png.dtype == np.uint8
        inside = np.zeros(src.shape[:2], dtype=bool)
        for name, y0, x0, y1, x1 in rows:
            if name == n:
                inside[max(y0, 0):y1, max(x0, 0):x1] = True
        assert np.array_equal(png[~inside], src[~inside]), n
        if inside.any():
            assert (png[inside] != src[inside]).mean() > 0.5, n
    # pose photos and their boxes, paired by row
    pose_boxes = str(tmp_path / 'poses.csv')
    with open(pose_boxes, 'w') as f:
        f.write(''.join('%s,%d,%d,%d,%d\n' % (names[k], 10, 10, 200, 160) for k in (1, 3, 4, 1)))
    out2 = str(tmp_path / 'reposed2')
    _run_script(os.path.join(ROOT, 'scripts', 'generate.py'), ['--configs', conf, '--checkpoint', ckpt, '--appearance-dir', imdir, '--boxes', boxes,
                                                               '--pose-dir', imdir, '--pose-boxes', pose_boxes, '--out-dir', out2, '--feather', '0',
                                                               '--batch-size', '4'])
    assert len(os.listdir(out2)) == 6
