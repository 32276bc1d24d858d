"""Compose, host side (no GPU): the ABI of imm_compose_u8 and its argument validation, the two numpy restatements of its pixel rule
against each other (tests/compose_reference.py) and the properties of the f32 one, the host logic of ImageGenerator.repose (the row
chain, the ramp reciprocals, the refusals) and the script surface."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compose_reference as R                                              # noqa: E402

from imm_amd import generation as G                                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = R.S_KERNEL
FEATHERS = (0.0, 0.125, 0.5)


# ----------------------------------------------------------------------------------------------------------------------------
# ABI and validation
# ----------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_compose_entry_point():
    from imm_amd import _lib as L
    assert L.ABI_VERSION >= 26
    assert L.symbols('imm_compose.h') == ['imm_compose_u8']


def test_compose_validates_its_arguments_without_a_device():
    from imm_amd import _lib as L
    lib = L.load()
    one = C.c_void_p(16)                                   # a non-null pointer that is never read: validation comes first
    good = [one, one, one, 1, one, one, one, one, 3, 1, 16, 256, None]
    for i, bad in ((0, None), (1, None), (2, None), (4, None), (5, None), (6, None), (7, None),      # null pointers
                   (3, 0), (8, 2), (9, 0), (9, 65536), (10, 0), (10, 8193), (11, 0)):                 # n_images, ld, n, image_size, max_box_pixels
        args = list(good)
        args[i] = bad
        assert lib.imm_compose_u8(*args) == -1, (i, bad)
        assert b'compose_u8' in lib.imm_last_error()


# ----------------------------------------------------------------------------------------------------------------------------
# the two restatements
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ld', [3, 4])
@pytest.mark.parametrize('feather', FEATHERS)
def test_f32_restatement_against_f64(feather, ld):
    photos, rows, faces = R.kernel_case(ld=ld)
    ramp = G.compose_inv_ramp(rows, feather)
    a = R.compose_f32(photos, rows, faces, ramp, S)
    b = R.compose_f64(photos, rows, faces, ramp, S)
    masks = R.box_mask(photos, rows)
    n_box = sum(int(m.sum()) for m in masks) * 3
    diff = np.concatenate([np.abs(x.astype(np.int64) - y.astype(np.int64)).reshape(-1) for x, y in zip(a, b)])
    print('\nCOMPOSE f32 vs f64 feather=%g ld=%d: %d of %d box bytes differ (max %d)' % (feather, ld, int((diff > 0).sum()), n_box,
                                                                                        int(diff.max())))
    assert diff.max() <= 1
    assert (diff > 0).sum() <= 0.005 * n_box
    for x, y, p, m in zip(a, b, photos, masks):
        assert np.array_equal(x[~m], p[~m]) and np.array_equal(y[~m], p[~m])         # nothing outside a box moves
    assert np.array_equal(a[3], photos[3]) and not masks[3].any()                     # the photo without a box
    assert not masks[1][0, 0] and masks[1].sum() > 0
    changed = sum(int((x != p).sum()) for x, p in zip(a, photos))
    assert changed > 0.5 * n_box                                                       # the faces did land


def test_identity_scale_with_the_float_crop_returns_the_photo():
    rng = np.random.RandomState(1)
    photo = rng.randint(0, 256, size=(31, 45, 3)).astype(np.uint8)
    rows = np.array([(0, 7, 11, 7 + S, 11 + S)], dtype=np.int32)
    faces = R.float_crop(photo, rows[0, 1:], S)[None]
    for feather in (0.0, 0.1, 0.25, 0.5):
        out = R.compose_f32([photo], rows, faces, G.compose_inv_ramp(rows, feather), S)
        assert np.array_equal(out[0], photo), feather


def test_feather_zero_is_a_hard_paste():
    photos, rows, faces = R.kernel_case()
    rows, faces = rows[:1], faces[:1]                                                  # the 16 x 16 box: g is the face pixel itself
    ramp = G.compose_inv_ramp(rows, 0.0)
    assert np.array_equal(ramp, np.full((1, 2), 2.0, np.float32))
    out = R.compose_f32(photos, rows, faces, ramp, S)
    _i, y0, x0, y1, x1 = rows[0]
    want = np.rint(np.clip(faces[0, :, :, :3], 0, 255)).astype(np.uint8)
    assert np.array_equal(out[0][y0:y1, x0:x1], want)
    assert (want == 0).any() and (want == 255).any()                                   # values clipped at both ends


def test_row_order_matters_on_an_overlap():
    photos, rows, faces = R.kernel_case()
    i, j = R.OVERLAPPING[1], R.OVERLAPPING[2]                                          # A (10..30, 10..30) and B (5..25, 20..38)
    pair, swapped = [i, j], [j, i]
    for feather in (0.0, 0.125):
        a = R.compose_f32(photos, rows[pair], faces[pair], G.compose_inv_ramp(rows[pair], feather), S)[1]
        b = R.compose_f32(photos, rows[swapped], faces[swapped], G.compose_inv_ramp(rows[swapped], feather), S)[1]
        both = np.zeros((40, 40), dtype=bool)
        both[10:25, 20:30] = True
        assert (a[both] != b[both]).mean() > 0.5
        assert np.array_equal(a[~both], b[~both])


# ----------------------------------------------------------------------------------------------------------------------------
# host logic
# ----------------------------------------------------------------------------------------------------------------------------
def test_next_row_chain_of_shuffled_rows():
    rng = np.random.RandomState(3)
    owner = rng.randint(0, 5, size=40)
    rows = np.stack([owner] + [np.zeros(40, np.int64)] * 2 + [np.ones(40, np.int64)] * 2, axis=1)
    links = G.compose_links(rows)
    assert links.dtype == np.int32 and links.shape == (40, 2)
    for b in range(40):
        later = [j for j in range(b + 1, 40) if owner[j] == owner[b]]
        earlier = [j for j in range(b) if owner[j] == owner[b]]
        assert links[b, 1] == (later[0] if later else -1)
        assert links[b, 0] == (earlier[-1] if earlier else -1)
    # the chain of a photo visits each of its rows once, in row order
    for img in range(5):
        mine = [b for b in range(40) if owner[b] == img]
        walk, b = [], mine[0]
        while b >= 0:
            walk.append(b)
            b = links[b, 1]
        assert walk == mine
    assert np.array_equal(G.compose_links(np.array(R.KERNEL_ROWS))[[2, 4, 6, 9, 10], 1], [4, 6, 9, 10, -1])
    assert G.compose_links(np.zeros((0, 5), np.int64)).shape == (0, 2)


def test_inv_ramp():
    rows = np.array([(0, 0, 0, 4, 100), (0, 0, 0, 1, 250), (0, -10, 5, 30, 6)], dtype=np.int32)          # sides (4, 100), (1, 250), (40, 1)
    r = G.compose_inv_ramp(rows, 0.125)
    assert r.dtype == np.float32 and r.shape == (3, 2)
    np.testing.assert_array_equal(r, np.array([[2.0, 1 / 12.5], [2.0, 1 / 31.25], [1 / 5.0, 2.0]], dtype=np.float32))
    assert (G.compose_inv_ramp(rows, 0.0) == 2.0).all()
    assert G.compose_inv_ramp(np.array([(0, 0, 0, 5, 4)]), 0.125)[0].tolist() == [np.float32(1 / 0.625), 2.0]   # 0.625 > 0.5, 0.5 is not
    # a value >= 2 makes every weight 1: (min(d, ...) + 0.5) * 2 >= 1 for d >= 0
    for bad in (-0.01, 0.51, float('nan')):
        with pytest.raises(ValueError):
            G.compose_inv_ramp(rows, bad)


def test_repose_refusals():
    K = 10
    photos = [np.zeros((30, 40, 3), np.uint8), np.zeros((20, 25), np.uint8)]
    boxes = [(0, 2, 3, 20, 30), (1, 0, 0, 20, 25), (1, -5, -5, 10, 10)]
    lm = torch.zeros(3, K, 2)
    ph, rows, pose, f = G.plan_repose(photos, lm, boxes, None, 0.125, K)
    assert rows.shape == (3, 5) and pose[0] == 'landmarks' and f == 0.125 and ph[1].shape == (20, 25, 3)
    assert len(G.plan_repose(photos, torch.zeros(1, K, 2), None, None, 0.0, K)[1]) == 2          # whole-photo boxes, one pose for all
    with pytest.raises(ValueError, match='boxes need the images as a list of u8 arrays'):
        G.plan_repose(torch.zeros(2, 128, 128, 3), lm, None, None, 0.125, K)
    for bad in (-0.1, 0.6, float('nan')):
        with pytest.raises(ValueError, match='feather'):
            G.plan_repose(photos, lm, boxes, None, bad, K)
    with pytest.raises(ValueError, match='poses'):
        G.plan_repose(photos, torch.zeros(2, K, 2), boxes, None, 0.125, K)                         # neither n nor 1
    with pytest.raises(ValueError, match='poses'):
        G.plan_repose(photos, torch.zeros(3, K + 1, 2), boxes, None, 0.125, K)
    pose_photos = [np.zeros((50, 50, 3), np.uint8)] * 2
    with pytest.raises(ValueError, match='2 poses for 3 faces'):
        G.plan_repose(photos, pose_photos, boxes, None, 0.125, K)
    assert G.plan_repose(photos, pose_photos, boxes, [(0, 0, 0, 9, 9), (1, 0, 0, 9, 9), (1, 5, 5, 50, 50)], 0.125, K)[2][0] == 'photos'
    assert G.plan_repose(photos, pose_photos[:1], boxes, None, 0.125, K)[2][0] == 'photos'
    with pytest.raises(ValueError, match='pose_boxes'):
        G.plan_repose(photos, lm, boxes, [(0, 0, 9, 9)] * 3, 0.125, K)
    with pytest.raises(ValueError):
        G.plan_repose(photos, lm, [(2, 0, 0, 5, 5)] * 3, None, 0.125, K)                           # check_boxes: no such photo


def test_generate_script_lists_the_repose_arguments():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'generate.py'), '--help'], cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-1500:]
    text = out.stdout.decode()
    for flag in ('--boxes', '--pose-boxes', '--out-dir', '--feather'):
        assert flag in text, flag
