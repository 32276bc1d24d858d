"""Annotation on the MI355X: imm_annotate_points bit for bit against the f64 restatement, imm_annotate_u8 in guarded buffers against the
numpy restatement of include/imm_annotate.h (tests/annotate_reference.py) BYTE FOR BYTE (every operation of the rule is reproduced in
numpy, so no cap is needed), the properties (a) to (i) of the rule checked on the device without the restatement, LandmarkDetector.annotate
and annotate_clip end to end, and the script."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alignment_reference as AR                  # noqa: E402
import annotate_reference as AN                   # noqa: E402
import guarded                                    # noqa: E402
import hull_reference as HR                       # noqa: E402
import test_detector_gpu as D                     # noqa: E402  (make_model, _run_script, _write_config)
from dataset_fixtures import make_celeba_tree     # noqa: E402
from test_colour_gpu import _count_calls          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
GRID_PIXELS = 4096               # max_box_pixels of the kernel tests: it sizes the grid only, larger extents are walked by the same grid
POINTS, BOX, HULL, LABEL, ALL = AN.POINTS, AN.BOX, AN.HULL, AN.LABEL, AN.ALL


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


@pytest.fixture(autouse=True)
def _guards_intact():
    guarded.reset()
    yield
    guarded.check_guards()


def gin(a):
    return guarded.inp(torch.from_numpy(np.array(a, order='C')), DEV, depth=2)      # (a copy: the shared references are read only)


PHOTOS = AN.photos_of()


def run_annotate(ops, photos, rows, bits, thickness, pad, scale, palette=AN.PALETTE, marks=None, gstyle=None, mstyle=None, edges=None,
                 status=None, labels=None, launches=None, max_pixels=GRID_PIXELS):
    """imm_annotate_u8 over a guarded copy of the packed photos -> (the photos, the whole buffer).  launches: [(a, b)] row ranges, each
    launched with the links of its own rows (generation.compose_links)."""
    from imm_amd.generation import compose_links
    buf, offs, hw = AN.pack(photos)
    rows = np.asarray(rows, np.int32).reshape(-1, 5)
    dst = guarded.out(buf.shape, torch.uint8, DEV, fill=torch.from_numpy(buf))
    offs_d, hw_d, rows_d, pal_d = gin(offs), gin(hw), gin(rows), gin(np.asarray(palette, np.uint8))
    marks = None if marks is None else np.asarray(marks, F32)
    gs_d = None if gstyle is None else gin(np.asarray(gstyle, F32))
    ms_d = None if mstyle is None else gin(np.asarray(mstyle, np.uint8))
    edges_d = None if edges is None else gin(np.asarray(edges, F32))
    status_d = None if status is None else gin(np.asarray(status, np.int32))
    labels_d = None if labels is None else gin(np.asarray(labels, np.int32))
    for a, b in launches or [(0, len(rows))]:
        cut = lambda t: None if t is None else t[a:b]
        ops.annotate_u8(dst, offs_d, hw_d, rows_d[a:b], gin(compose_links(rows[a:b])), pal_d, bits, thickness, pad, scale, max_pixels,
                        marks=None if marks is None else gin(marks[:, a:b]), group_style=gs_d, mark_style=ms_d, edges=cut(edges_d),
                        status=cut(status_d), labels=cut(labels_d))
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    return AN.unpack(got, photos), got


def same_photos(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere((g != w).any(axis=2))
        assert not len(bad), '%s: photo %d differs at %d pixels, first (%d, %d): got %s want %s' % (
            what, i, len(bad), bad[0][0], bad[0][1], g[tuple(bad[0])], w[tuple(bad[0])])


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the points, bit for bit
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 65])
def test_points_kernel_equals_the_f64_restatement_bit_for_bit(ops, n):
    for K in (1, 10, 80):
        rng = np.random.RandomState(n + K)
        rows = AN.case_rows(n).copy()
        mu = rng.uniform(-1.2, 1.2, (n, K, 2)).astype(F32)
        mu[n - 1, K // 2] = (-1.0, 1.0)                                      # the box's own corners
        if n >= 3:
            rows[1, 1:] = (7, 9, 7, 30)                                      # an empty box
            rows[2, 1:] = (30, 10, 20, 5)                                    # an inverted box
            mu[1, 0, 0], mu[2, K - 1, 1] = np.inf, np.nan
        mu[0, 0, 1], mu[0, K - 1, 0] = np.nan, -np.inf
        out = guarded.out((n, K, 2), torch.float32, DEV)
        mu_d = gin(mu)
        ops.annotate_points(mu_d, gin(rows), out)
        torch.cuda.synchronize()
        got, want = out.cpu().numpy(), AN.points(mu, rows)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert not len(bad), 'n %d K %d: %d values differ, first %s: got %r want %r' % (n, K, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
        assert np.array_equal(mu_d.cpu().numpy().view(np.uint32), mu.view(np.uint32)), 'mu is read only'
        keep = ~np.isfinite(mu)
        assert keep.sum() >= 2 and np.array_equal(got.view(np.uint32)[keep], mu.view(np.uint32)[keep]), 'what is not finite is stored as it is'


# ----------------------------------------------------------------------------------------------------------------------------
# 2. the paste against the restatement, byte for byte
# ----------------------------------------------------------------------------------------------------------------------------
# (K, G, draw bits, thickness, size, pad, label_scale): every draw bit alone and all together, K in {1, 10, 57}, G in {1, 4}, thickness in
# {1, 3}, size in {1, 2.5, 6}, pad in {0, 8}, label_scale in {1, 2}
CONFIGS = [(10, 1, POINTS, 1, 2.5, 8, 1), (10, 1, BOX, 1, 2.5, 0, 1), (10, 1, HULL, 1, 2.5, 8, 1), (10, 1, LABEL, 1, 2.5, 0, 1),
           (10, 4, ALL, 3, 6.0, 8, 2), (57, 1, ALL, 1, 1.0, 0, 1), (57, 4, POINTS, 3, 2.5, 8, 1), (1, 1, ALL, 3, 2.5, 8, 2),
           (1, 4, POINTS | BOX, 1, 6.0, 0, 1), (10, 1, HULL | BOX, 3, 1.0, 0, 2), (10, 4, ALL, 1, 1.0, 8, 1), (10, 1, BOX | LABEL, 3, 2.5, 0, 2)]


def case_hull(rows, K, seed=5):
    """imm_hull_fit's lines (tests/hull_reference.py) for random clouds in the rows, one row flagged (a NaN landmark), and wild values (NaN,
    inf, 1e30) in single lines of later rows."""
    rows = np.asarray(rows).reshape(-1, 5)
    n = len(rows)
    rng = np.random.RandomState(seed + n + K)
    poses = rng.uniform(-0.9, 0.9, (n, K, 2)).astype(F32)
    if n > 1:
        poses[1, 0, 0] = np.nan
    edges, flags = HR.hull_fit(poses, rows, np.full(n, 1.25, F32))
    edges = edges.copy()
    for i, b in enumerate(range(4, n, 9)):
        edges[b, i % K, i % 3] = (np.nan, np.inf, -np.inf, 1e30, -1e30)[i % 5]
    return edges, flags


def case_inputs(n, K, G, bits, size, pad):
    rows = AN.case_rows(n)
    kw = dict(status=AN.case_status(n))
    if bits & POINTS:
        kw.update(marks=AN.case_marks(rows, K, G, pad), gstyle=AN.group_styles(size, G, 1.0 if K == 10 else 0.6), mstyle=AN.mark_styles(K))
    if bits & HULL:
        kw.update(edges=case_hull(rows, K)[0])
    if bits & LABEL:
        kw.update(labels=AN.case_labels(n))
    return rows, kw


@pytest.mark.parametrize('n', [1, 3, 65])
def test_paste_kernel_equals_the_restatement_byte_for_byte(ops, n):
    for K, G, bits, thickness, size, pad, scale in CONFIGS:
        rows, kw = case_inputs(n, K, G, bits, size, pad)
        what = 'n %d K %d G %d bits %d thickness %d size %g pad %d scale %d' % (n, K, G, bits, thickness, size, pad, scale)
        want, covered, drawn = AN.annotate(PHOTOS, rows, bits, thickness, pad, scale, **kw)
        got, buf = run_annotate(ops, PHOTOS, rows, bits, thickness, pad, scale, **kw)
        same_photos(got, want, what)
        # the padding between the photos, and every byte outside every extent (the restatement leaves both alone)
        assert np.array_equal(buf, AN.pack(want)[0]), what
        for g, p, cov in zip(got, PHOTOS, covered):
            assert np.array_equal(g[~cov], p[~cov]), what
        assert any(d.any() for d in drawn) or n == 1, what
    if n == 65:                                             # the grid sized by the largest extent itself (capped at 2^31 - 1 pixels)
        from imm_amd.annotation import grid_pixels
        K, G, bits, thickness, size, pad, scale = CONFIGS[4]
        rows, kw = case_inputs(n, K, G, bits, size, pad)
        got, _buf = run_annotate(ops, PHOTOS, rows, bits, thickness, pad, scale, max_pixels=grid_pixels(rows, pad), **kw)
        same_photos(got, AN.annotate(PHOTOS, rows, bits, thickness, pad, scale, **kw)[0], 'the full grid')
        # no status: every frame in palette[0]
        kw.pop('status')
        got, _buf = run_annotate(ops, PHOTOS, rows, bits, thickness, pad, scale, **kw)
        same_photos(got, AN.annotate(PHOTOS, rows, bits, thickness, pad, scale, **kw)[0], 'status NULL')


# ----------------------------------------------------------------------------------------------------------------------------
# 3. properties that do not lean on the restatement
# ----------------------------------------------------------------------------------------------------------------------------
def one_mark(ops, photo, row, at, k=1, size=2.5, alpha=1.0):
    """One row with one marker of style k at `at` over `photo`: the drawn photo."""
    marks = np.array(at, F32).reshape(1, 1, 1, 2)
    return run_annotate(ops, [photo], [row], POINTS, 1, 8, 1, marks=marks, gstyle=AN.group_styles(size, 1, alpha),
                        mstyle=AN.mark_styles(k + 1)[k:k + 1])[0][0]


def test_a_no_draw_bit_returns_the_photos(ops):
    n = len(AN.ROWS)
    rows, kw = case_inputs(n, 10, 2, ALL, 2.5, 8)
    _got, buf = run_annotate(ops, PHOTOS, rows, 0, 3, 8, 2, **kw)
    assert np.array_equal(buf, AN.pack(PHOTOS)[0])


def test_b_the_pixel_under_a_marker_is_its_colour_and_c_far_pixels_keep_their_bytes(ops):
    photo = PHOTOS[1]
    row = (0, 10, 10, 50, 60)
    styles = AN.mark_styles(56)
    for k in range(0, 56, 3):
        for size in (2.5, 6.0):
            out = one_mark(ops, photo, row, (30, 35), k, size)
            assert out[30, 35].tolist() == styles[k, :3].tolist(), (k, size)
            r, c = np.nonzero((out != photo).any(axis=2))
            assert len(r) and np.maximum(np.abs(r - 30), np.abs(c - 35)).max() <= size + 2, (k, size)
    # (c) with many marks, a frame, a hull and a label: a pixel farther than R + 2 from every mark and on no other primitive keeps its byte
    rows = np.array([(1, 6, 8, 58, 72)], np.int32)
    marks = np.random.RandomState(3).uniform(10, 55, (3, 1, 10, 2)).astype(F32)
    poses = np.random.RandomState(4).uniform(-0.7, 0.7, (1, 10, 2)).astype(F32)
    edges, flags = HR.hull_fit(poses, rows, np.full(1, 1.0, F32))
    assert flags[0] == 0
    kw = dict(marks=marks, gstyle=AN.group_styles(2.5, 3), mstyle=styles[:10], labels=[12], edges=edges)
    got = run_annotate(ops, PHOTOS, rows, ALL, 2, 6, 1, **kw)[0][1]
    others = run_annotate(ops, PHOTOS, rows, ALL & ~POINTS, 2, 6, 1, **kw)[0][1]
    r, c = np.mgrid[0:64, 0:80]
    cheb = np.min([np.maximum(np.abs(r - my), np.abs(c - mx)) for my, mx in marks.reshape(-1, 2).astype(np.float64)], axis=0)
    far = (cheb > 2.5 + 2) & (others == PHOTOS[1]).all(axis=2)
    assert far.sum() > 500 and np.array_equal(got[far], PHOTOS[1][far]) and (got != others).any()


def test_d_the_frame_is_the_integer_ring_in_the_colour_of_the_status(ops):
    photo = PHOTOS[1]
    y0, x0, y1, x1 = 8, 12, 40, 70
    for thickness in (1, 3):
        ring = np.zeros(photo.shape[:2], bool)
        ring[y0:y1, x0:x1] = True
        ring[y0 + thickness:y1 - thickness, x0 + thickness:x1 - thickness] = False
        for status, colour in ((None, 0), (0, 0), (1, 1), (2, 2), (4, 3), (6, 2), (5, 1), (1 << 20, 3), (-2 ** 31, 3)):
            out = run_annotate(ops, [photo], [(0, y0, x0, y1, x1)], BOX, thickness, 8, 1, status=None if status is None else [status])[0][0]
            assert (out[ring] == AN.PALETTE[colour]).all() and np.array_equal(out[~ring], photo[~ring]), (thickness, status)


def test_e_a_lost_row_draws_its_frame_and_label_only_and_f_a_flagged_hull_draws_nothing(ops):
    photo = PHOTOS[1]
    rows = np.array([(0, 8, 12, 48, 70)], np.int32)
    marks = AN.case_marks(rows, 10, 2, 5)
    poses = np.random.RandomState(1).uniform(-0.8, 0.8, (1, 10, 2)).astype(F32)
    edges, flags = HR.hull_fit(poses, rows, np.full(1, 1.25, F32))
    assert flags[0] == 0
    kw = dict(marks=marks, gstyle=AN.group_styles(2.5, 2), mstyle=AN.mark_styles(10), labels=[42], edges=edges)
    full = run_annotate(ops, [photo], rows, ALL, 2, 5, 1, status=[0], **kw)[0][0]
    lost = run_annotate(ops, [photo], rows, ALL, 2, 5, 1, status=[1], **kw)[0][0]
    only = run_annotate(ops, [photo], rows, BOX | LABEL, 2, 5, 1, status=[1], labels=[42])[0][0]
    assert np.array_equal(lost, only) and not np.array_equal(full, lost)
    ring = np.zeros(photo.shape[:2], bool)
    ring[8:48, 12:70] = True
    ring[10:46, 14:68] = False
    ring[10:10 + 9, 14:14 + 13] = True                                       # the label's rectangle: two digits
    assert np.array_equal(lost[~ring], photo[~ring]) and (lost[8, 12:70] == AN.PALETTE[1]).all()
    # (f) a flagged hull
    hull = run_annotate(ops, [photo], rows, HULL, 2, 5, 1, edges=edges)[0][0]
    assert (hull != photo).any() and (hull[28, 40] == photo[28, 40]).all()
    bad = poses.copy()
    bad[0, 3, 1] = np.nan
    e2, f2 = HR.hull_fit(bad, rows, np.full(1, 1.25, F32))
    assert f2[0] & 1 and np.isneginf(e2[0, :, 2]).all()
    assert np.array_equal(run_annotate(ops, [photo], rows, HULL, 2, 5, 1, edges=e2)[0][0], photo)


def test_g_marks_on_a_pixel_centre_are_symmetric_and_up_is_down_flipped(ops):
    flat = np.full((41, 41, 3), 90, np.uint8)
    row = (0, 2, 2, 39, 39)
    for size in (1.0, 2.5, 6.0):
        patch = {AN.SHAPES[k // 8]: one_mark(ops, flat, row, (20, 20), k, size).astype(int) - 90 for k in range(0, 56, 8)}
        for shape, p in patch.items():
            assert p.any(), (shape, size)
            if shape in 'osd+x':
                assert np.array_equal(p, p[::-1]) and np.array_equal(p, p[:, ::-1]), (shape, size)
            else:
                assert np.array_equal(p, p[:, ::-1]) and not np.array_equal(p, p[::-1]), (shape, size)
        same = AN.mark_styles(40)
        same[32, :3] = same[0, :3]
        at = np.array([20, 20], F32).reshape(1, 1, 1, 2)
        v = run_annotate(ops, [flat], [row], POINTS, 1, 8, 1, marks=at, gstyle=AN.group_styles(size, 1), mstyle=same[0:1])[0][0]
        up = run_annotate(ops, [flat], [row], POINTS, 1, 8, 1, marks=at, gstyle=AN.group_styles(size, 1), mstyle=same[32:33])[0][0]
        assert np.array_equal(v, up[::-1]) and (v != flat).any(), size


def test_h_disjoint_rows_one_by_one_give_the_bytes_of_one_launch(ops):
    # the extents (pad 4) of these rows are disjoint, two of them in one photo
    rows = np.array([(1, 5, 5, 30, 30), (1, 34, 40, 60, 75), (0, 6, 6, 30, 40), (1, 5, 45, 25, 74)], np.int32)
    n = len(rows)
    marks = AN.case_marks(rows, 10, 2, 4)
    kw = dict(marks=marks, gstyle=AN.group_styles(2.5, 2), mstyle=AN.mark_styles(10), labels=AN.case_labels(n), status=[0, 2, 4, 1],
              edges=case_hull(rows, 10)[0])
    _p, whole = run_annotate(ops, PHOTOS, rows, ALL, 2, 4, 1, **kw)
    assert not np.array_equal(whole, AN.pack(PHOTOS)[0])
    for launches in ([(0, 2), (2, n)], [(i, i + 1) for i in range(n)]):
        _p, parts = run_annotate(ops, PHOTOS, rows, ALL, 2, 4, 1, launches=launches, **kw)
        assert np.array_equal(parts, whole), len(launches)


def test_i_the_later_of_two_overlapping_rows_lies_over_the_earlier(ops):
    two = np.array([(1, 10, 10, 40, 40), (1, 20, 20, 50, 50)], np.int32)
    out = run_annotate(ops, PHOTOS, two, BOX, 2, 0, 1, status=[0, 1])[0][1]
    assert (out[20, 25] == AN.PALETTE[1]).all() and (out[39, 25] == AN.PALETTE[0]).all() and (out[20, 39] == AN.PALETTE[1]).all()
    out = run_annotate(ops, PHOTOS, two[::-1].copy(), BOX, 2, 0, 1, status=[1, 0])[0][1]
    assert (out[20, 39] == AN.PALETTE[0]).all() and (out[20, 25] == AN.PALETTE[1]).all()
    # a marker of the later row over the frame of the earlier, and a marker of the earlier under the frame of the later
    marks = np.array([[[(20, 30)], [(39, 30)]]], F32)                        # [1, 2, 1, 2]: row 0's mark on row 1's frame, and back
    kw = dict(marks=marks, gstyle=AN.group_styles(2.5, 1), mstyle=AN.mark_styles(2)[1:2], status=[0, 2])
    out = run_annotate(ops, PHOTOS, two, POINTS | BOX, 2, 4, 1, **kw)[0][1]
    assert (out[20, 30] == AN.PALETTE[2]).all(), 'the later row frames over the earlier row\'s marker'
    assert out[39, 30].tolist() == AN.mark_styles(2)[1, :3].tolist(), 'the later row\'s marker lies over the earlier row\'s frame'


# ----------------------------------------------------------------------------------------------------------------------------
# 4. LandmarkDetector.annotate
# ----------------------------------------------------------------------------------------------------------------------------
SCENE_SIZES = [(150, 131), (120, 163)]
SCENE_BOXES = [(0, 10, 12, 100, 90), (1, 5, 20, 90, 101), (0, 60, 50, 160, 140)]
GROW = 16.0                      # the landmarks of a model with random weights lie within a pixel or two of each other


@pytest.fixture(scope='module')
def world(ops):
    cfg, model, eng, P, St = D.make_model(10, 128, 2)
    return dict(model=model, eng=eng, det=model.landmark_detector(128, max_batch=2),
                photos=[AR.smooth_photo(h, w, 40 + i) for i, (h, w) in enumerate(SCENE_SIZES)])


def host(t):
    return t.cpu().numpy()


def test_detector_annotate_equals_the_restatement_on_its_own_landmarks(ops, world):
    det, photos = world['det'], world['photos']
    rows = np.array(SCENE_BOXES, np.int32)
    n = len(rows)
    mu = host(det.landmarks(photos, SCENE_BOXES))
    pts = AN.points(mu, rows)
    det.annotate(photos, SCENE_BOXES)                                                          # (captures out of the way)
    (out, tr), calls = _count_calls(ops, lambda: det.annotate(photos, SCENE_BOXES, return_transform=True))
    # n = 3 rows at max_batch 2: two buckets of the pose program, then ONE launch each of the points and the paste
    assert calls.count('imm_resize_crop_u8') == 2 and calls.count('imm_annotate_points') == 1 == calls.count('imm_annotate_u8')
    assert 'imm_hull_fit' not in calls
    assert np.array_equal(host(tr.points).view(np.uint32), pts.view(np.uint32)) and tr.hull_edges is None
    want, _cov, drawn = AN.annotate(photos, rows, POINTS | BOX, 1, 5, 1, marks=pts[None], gstyle=AN.group_styles(2.5, 1), mstyle=AN.mark_styles(10))
    assert all(o.is_cuda and o.dtype == torch.uint8 for o in out)
    same_photos([host(o) for o in out], want, 'annotate, the defaults')
    assert all(d.any() for d in drawn)
    # everything drawn, with a status and labels
    status = [0, 4, 1]
    kw = dict(draw=('points', 'box', 'hull', 'label'), size=6.0, thickness=3, status=status, labels=[7, 42, 1234], grow=GROW, alpha=0.5,
              label_scale=2)
    (out, tr), calls = _count_calls(ops, lambda: det.annotate(photos, SCENE_BOXES, return_transform=True, **kw))
    assert calls.count('imm_hull_fit') == 1 == calls.count('imm_annotate_u8')
    edges, flags = HR.hull_fit(mu, rows, np.full(n, GROW, F32))
    assert np.array_equal(host(tr.hull_edges).view(np.uint32), edges.view(np.uint32)) and np.array_equal(host(tr.hull_flags), flags)
    want, _cov, _d = AN.annotate(photos, rows, ALL, 3, 8, 2, marks=pts[None], gstyle=AN.group_styles(6.0, 1, 0.5), mstyle=AN.mark_styles(10),
                                 edges=edges, status=status, labels=[7, 42, 1234])
    same_photos([host(o) for o in out], want, 'annotate, everything')
    # labels=None numbers the rows
    out = det.annotate(photos, SCENE_BOXES, draw=('label',))
    want, _cov, _d = AN.annotate(photos, rows, LABEL, 1, 5, 1, labels=np.arange(n))
    same_photos([host(o) for o in out], want, 'annotate, numbered')


def test_detector_annotate_with_landmarks_runs_no_pose_program(ops, world):
    det, photos = world['det'], world['photos']
    rows = np.array(SCENE_BOXES, np.int32)
    lm = np.random.RandomState(4).uniform(-0.8, 0.8, (len(rows), 10, 2)).astype(F32)
    lm[1, 4, 1] = np.nan
    (out, tr), calls = _count_calls(ops, lambda: det.annotate(photos, SCENE_BOXES, landmarks=lm, draw=('points', 'hull'), return_transform=True))
    assert calls == ['imm_annotate_points', 'imm_hull_fit', 'imm_annotate_u8'], calls
    pts = AN.points(lm, rows)
    edges, flags = HR.hull_fit(lm, rows, np.full(len(rows), 1.25, F32))
    assert [int(f) & 1 for f in flags] == [0, 1, 0] and np.array_equal(host(tr.hull_flags), flags)
    want, _cov, _d = AN.annotate(photos, rows, POINTS | HULL, 1, 5, 1, marks=pts[None], gstyle=AN.group_styles(2.5, 1), mstyle=AN.mark_styles(10),
                                 edges=edges)
    same_photos([host(o) for o in out], want, 'annotate with landmarks=')
    _out, calls = _count_calls(ops, lambda: det.annotate(photos, SCENE_BOXES, draw=('box',)))
    assert calls == ['imm_annotate_u8'], calls


# ----------------------------------------------------------------------------------------------------------------------------
# 5. LandmarkDetector.annotate_clip
# ----------------------------------------------------------------------------------------------------------------------------
FACES = [(20, 24, 110, 100), (40, 120, 120, 190)]


def clip_frames(T=5):
    """Five frames cut from one photo, the cut moving so that what lies under the second face leaves through the right edge."""
    big = AR.smooth_photo(170, 330, 77)
    return [np.ascontiguousarray(big[8 - 2 * t:8 - 2 * t + 150, 30 * t:30 * t + 210]) for t in range(T)]


def _record_calls(ops, fn):
    """fn() with every library call of imm_amd.ops recorded with its arguments."""
    seen, call0 = [], ops.call
    ops.call = lambda name, *a: (seen.append((name, a)), call0(name, *a))[1]
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.call = call0
    return out, seen


def test_annotate_clip_equals_the_restatement_fed_with_its_track(ops, world):
    """Five frames, two faces, trail = 2.  A tracker over a model with random weights does not lose a face whose content leaves the
    photo (its landmarks stay finite: the frame only takes the colour of `outside` once the box itself has left), so the loss is made
    certain with a gate: its threshold lies between the two faces' mean spreads on frame 1, measured with an open gate, so that on
    frame 1 exactly one face is lost."""
    from imm_amd.annotation import ClipAnnotation
    from imm_amd.quality import QualityGate
    det, frames = world['det'], clip_frames()
    T, Fn = len(frames), len(FACES)
    scored = det.tracker(gate=QualityGate()).track(frames, FACES).cpu()
    sbar = scored.score[1, :, 0].numpy().astype(np.float64)
    assert sbar[0] != sbar[1]
    gate = QualityGate(max_spread=float(sbar.mean()))
    kw = dict(draw=('points', 'box', 'label'), trail=2, gate=gate, chunk_frames=3)
    det.annotate_clip(frames[:2], FACES, **kw)                                                 # (captures and allocations out of the way)
    ca, seen = _record_calls(ops, lambda: det.annotate_clip(frames, FACES, **kw))
    assert isinstance(ca, ClipAnnotation) and len(ca) == T and tuple(ca.status.shape) == (T, Fn)
    launches = [a for name, a in seen if name == 'imm_annotate_u8']
    assert len(launches) == T and [a[19] for a in launches] == [1, 2, 3, 3, 3], 'frames 0 and 1 use 1 and 2 groups'
    assert not any(name == 'imm_hull_fit' for name, _a in seen)
    tr = ca.track.cpu()
    boxes, pts, flags, qflags = tr.boxes.numpy(), tr.points_smooth.numpy(), tr.flags.numpy(), tr.qflags.numpy()
    status = flags | ((qflags != 0).astype(np.int32) << 2)
    assert np.array_equal(host(ca.status), status)
    lost = (flags & 1) != 0
    assert not lost[0].any() and lost[1].sum() == 1, 'on frame 1 exactly one face is lost'
    print('\nANNOTATE CLIP status per frame and face: %s' % status.tolist())
    for t in range(T):
        rows = np.concatenate([np.zeros((Fn, 1), np.int32), boxes[t]], axis=1)
        G = min(2, t) + 1
        want, covered, _d = AN.annotate([frames[t]], rows, POINTS | BOX | LABEL, 1, 5, 1, marks=pts[t + 1 - G:t + 1], gstyle=AN.group_styles(2.5, G),
                                        mstyle=AN.mark_styles(10), status=status[t], labels=np.arange(Fn))
        assert ca.frames[t].dtype == torch.uint8 and tuple(ca.frames[t].shape) == frames[t].shape
        same_photos([host(ca.frames[t])], want, 'frame %d' % t)
        for f in np.nonzero(lost[t])[0]:
            # the lost face: its frame in the lost colour, and inside it nothing but the label (one digit), away from the other face
            got = host(ca.frames[t])
            y0, x0, y1, x1 = (int(v) for v in boxes[t, f])
            oy0, ox0, oy1, ox1 = (int(v) for v in boxes[t, 1 - f])
            r, c = np.mgrid[0:got.shape[0], 0:got.shape[1]]
            box = (r >= y0) & (r < y1) & (c >= x0) & (c < x1)
            apart = ~((r >= oy0 - 5) & (r < oy1 + 5) & (c >= ox0 - 5) & (c < ox1 + 5))
            ring = box & ((r == y0) | (r == y1 - 1) | (c == x0) | (c == x1 - 1))
            label = (r >= y0 + 1) & (r < y0 + 10) & (c >= x0 + 1) & (c < x0 + 8)
            assert (ring & apart).any() and (got[ring & apart] == AN.PALETTE[1]).all(), 'the lost face is framed in the lost colour'
            inner = ~ring & ~label & apart
            assert (inner & box).any() and np.array_equal(got[inner], frames[t][inner]), 'a lost face draws no markers'
    # a Track the caller already has: the same bytes, and no tracker launch
    again, seen = _record_calls(ops, lambda: det.annotate_clip(frames, track=ca.track, draw=('points', 'box', 'label'), trail=2, chunk_frames=3))
    assert [name for name, _a in seen] == ['imm_annotate_u8'] * T
    assert all(torch.equal(a, b) for a, b in zip(again.frames, ca.frames)) and torch.equal(again.status, ca.status)
    host_track = det.annotate_clip(frames, track=tr, draw=('points', 'box', 'label'), trail=2)
    assert all(torch.equal(a, b) for a, b in zip(host_track.frames, ca.frames)), 'a Track on the host, one chunk'
    # the hull: one imm_hull_fit per frame, on the frame's own landmarks
    hull, calls = _count_calls(ops, lambda: det.annotate_clip(frames, track=ca.track, draw=('hull',), grow=GROW))
    assert calls == ['imm_hull_fit', 'imm_annotate_u8'] * T
    mu = tr.mu.numpy()
    for t in (0, T - 1):
        rows = np.concatenate([np.zeros((Fn, 1), np.int32), boxes[t]], axis=1)
        edges, _flags = HR.hull_fit(mu[t], rows, np.full(Fn, GROW, F32))
        want, _c, _d = AN.annotate([frames[t]], rows, HULL, 1, 5, 1, edges=edges, status=status[t])
        same_photos([host(hull.frames[t])], want, 'the hull of frame %d' % t)
    with pytest.raises(ValueError, match='exactly one'):
        det.annotate_clip(frames, FACES, track=ca.track)


# ----------------------------------------------------------------------------------------------------------------------------
# 6. the script
# ----------------------------------------------------------------------------------------------------------------------------
def test_detect_script_annotates(ops, world, tmp_path, capsys):
    from PIL import Image
    from imm_amd.inference import LandmarkDetector
    from imm_amd.utils.config import load_configs
    eng = world['eng']
    root = str(tmp_path / 'celeba')
    names, pixels = make_celeba_tree(root, n=4)
    ckpt = str(tmp_path / 'model.pt')
    torch.save({'params': eng.named_parameters(), 'state': eng.named_state()}, ckpt)
    conf = D._write_config(tmp_path, root, str(tmp_path / 'logs'))
    imdir = os.path.join(root, 'Img', 'img_align_celeba_hq')
    files = sorted(f for f in os.listdir(imdir) if f.lower().endswith(('.jpg', '.jpeg', '.png', '.bmp')))
    first = str(tmp_path / 'first.csv')
    faces = [(30, 20, 170, 140), (110, 70, 210, 170)]
    with open(first, 'w') as f:
        f.write(''.join('%s,%d,%d,%d,%d\n' % ((files[0],) + r) for r in faces))
    script = os.path.join(ROOT, 'scripts', 'detect.py')
    common = ['--configs', conf, '--checkpoint', ckpt, '--images-dir', imdir, '--batch-size', '4', '--boxes', first]
    det = LandmarkDetector.from_checkpoint(load_configs([conf]).model, ckpt, image_size=128, max_batch=4, device=DEV)
    photos = [pixels[f] for f in files]
    out_dir = str(tmp_path / 'clip')
    D._run_script(script, common + ['--track', '--annotate', '--draw', 'points,box,label', '--trail', '2', '--out-dir', out_dir])
    assert '4 frames, 2 faces annotated' in capsys.readouterr().out
    assert sorted(os.listdir(out_dir)) == [os.path.splitext(f)[0] + '.png' for f in files]
    ca = det.annotate_clip(photos, [list(r) for r in faces], draw=('points', 'box', 'label'), trail=2)
    for f, w, p in zip(files, ca.frames, photos):
        png = np.asarray(Image.open(os.path.join(out_dir, os.path.splitext(f)[0] + '.png')))
        assert np.array_equal(png, host(w)) and (png != p).any(), f
    # photos: --annotate over the boxes of a file
    out_dir = str(tmp_path / 'photos')
    D._run_script(script, common + ['--annotate', '--draw', 'points,box,hull', '--marker-size', '4', '--grow', '2', '--out-dir', out_dir])
    assert '2 faces annotated in 4 images' in capsys.readouterr().out
    want = det.annotate(photos, [(0,) + r for r in faces], draw=('points', 'box', 'hull'), size=4.0, grow=2.0)
    for f, w in zip(files, want):
        assert np.array_equal(np.asarray(Image.open(os.path.join(out_dir, os.path.splitext(f)[0] + '.png'))), host(w)), f
    with pytest.raises(ValueError, match='--out-dir'):
        D._run_script(script, common + ['--annotate'])
    with pytest.raises(ValueError, match='--redact'):
        D._run_script(script, common + ['--annotate', '--redact', 'pixelate', '--out-dir', out_dir])
