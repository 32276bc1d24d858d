"""Redaction on the MI355X: imm_redact_cells_u8 and imm_redact_u8 in guarded buffers against the numpy restatement of
include/imm_redact.h (tests/redact_reference.py) BYTE FOR BYTE (every operation of the rule is reproduced in numpy, so no cap is
needed), the fail-closed rule, the hull weight against tests/hull_reference.py bit for bit, split invariance, the header's consequences
(a) and (b), LandmarkDetector.redact and redact_clip end to end, and the script."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alignment_reference as AR                  # noqa: E402
import guarded                                    # noqa: E402
import hull_reference as HR                       # noqa: E402
import redact_reference as RR                     # noqa: E402
import test_detector_gpu as D                     # noqa: E402  (make_model, _run_script, _write_config)
from dataset_fixtures import make_celeba_tree     # noqa: E402
from test_colour_gpu import _count_calls          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
GRID_PIXELS = 4096               # max_box_pixels of the kernel tests: it sizes the grid only, larger boxes are walked by the same grid


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


PHOTOS = RR.photos_of()
_cells = {}


def ref_cells(n, blocks):
    """The restatement's cells of case_rows(n), computed once and shared (read only)."""
    if (n, blocks) not in _cells:
        _cells[n, blocks] = RR.cells_all(PHOTOS, RR.case_rows(n), blocks)
        _cells[n, blocks].setflags(write=False)
    return _cells[n, blocks]


def run_cells(ops, photos, rows, blocks, one_by_one=False):
    """imm_redact_cells_u8 over the packed photos, everything in guarded buffers, cells prefilled with 0xFF -> u8 [n, blocks^2 * 3]."""
    buf, offs, hw = RR.pack(photos)
    n = len(rows)
    src, offs_d, hw_d, rows_d = gin(buf), gin(offs), gin(hw), gin(np.asarray(rows, np.int32))
    cells = guarded.out((n, blocks * blocks * 3), torch.uint8, DEV)
    for a, b in ([(i, i + 1) for i in range(n)] if one_by_one else [(0, n)]):
        ops.redact_cells_u8(src, offs_d, hw_d, rows_d[a:b], blocks, cells[a:b])
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), buf), 'the photos are read only'
    return cells.cpu().numpy()


def run_paste(ops, photos, rows, cells, blocks, mode, feather, hull=None, launches=None, max_pixels=GRID_PIXELS):
    """imm_redact_u8 over a guarded copy of the packed photos -> (the photos, the whole buffer).  hull: (edges, inv_soft, flags);
    launches: [(a, b)] row ranges, each launched with the links of its own rows (generation.compose_links)."""
    from imm_amd.generation import compose_links
    buf, offs, hw = RR.pack(photos)
    rows = np.asarray(rows, np.int32)
    dst = guarded.out(buf.shape, torch.uint8, DEV, fill=torch.from_numpy(buf))
    offs_d, hw_d, rows_d, cells_d = gin(offs), gin(hw), gin(rows), gin(cells)
    ramp_d = gin(RR.inv_ramp(rows, feather))
    hull_d = None if hull is None else [gin(np.asarray(hull[0], F32)), gin(np.asarray(hull[1], F32)), gin(np.asarray(hull[2], np.int32))]
    for a, b in launches or [(0, len(rows))]:
        kw = {} if hull_d is None else dict(edges=hull_d[0][a:b], inv_soft=hull_d[1][a:b], hull_flags=hull_d[2][a:b])
        ops.redact_u8(dst, offs_d, hw_d, rows_d[a:b], gin(compose_links(rows[a:b])), ramp_d[a:b], cells_d[a:b], blocks, mode, max_pixels, **kw)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    return RR.unpack(got, photos), got


def same_photos(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere((g != w).any(axis=2))
        assert not len(bad), '%s: photo %d differs at %d pixels, first (%d, %d): got %s want %s' % (
            what, i, len(bad), bad[0][0], bad[0][1], g[tuple(bad[0])], w[tuple(bad[0])])


def box_is_its_means(out, photo, row, blocks, what):
    """Every pixel of the row's box that lies in the photo equals its cell's mean of the ORIGINAL photo."""
    row = [int(v) for v in row]
    cell, gy, gx = RR.grid(row, blocks)
    means = RR.cells(photo, row, blocks)[:gy * gx * 3].reshape(gy, gx, 3)
    px = RR._box_pixels(row, *photo.shape[:2])
    assert px is not None, what
    r, c = px
    assert np.array_equal(out[r, c], means[(r - row[1]) // cell, (c - row[2]) // cell]), what


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the cells, exact
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 65])
def test_cells_kernel_writes_the_whole_buffer_of_the_restatement(ops, n):
    rows = RR.case_rows(n)
    for blocks in RR.BLOCKS:
        want = ref_cells(n, blocks)
        got = run_cells(ops, PHOTOS, rows, blocks)
        bad = np.argwhere(got != want)
        assert not len(bad), 'blocks %d: %d bytes differ, first row %d byte %d: got %d want %d' % (
            blocks, len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])
        if n <= len(RR.ROWS) or blocks == 7:
            assert np.array_equal(run_cells(ops, PHOTOS, rows, blocks, one_by_one=True), want), 'rows launched one by one'
    if n == 65:
        assert any(w[:3].any() for w in ref_cells(n, 1)) and not ref_cells(n, 8)[10].any() and not ref_cells(n, 8)[15].any()


# ----------------------------------------------------------------------------------------------------------------------------
# 2. the paste without a mask, exact
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [RR.PIXELATE, RR.SMOOTH])
@pytest.mark.parametrize('n', [1, 3, 65])
def test_paste_kernel_equals_the_f32_restatement(ops, n, mode):
    rows = RR.case_rows(n)
    for blocks in RR.BLOCKS:
        cells = ref_cells(n, blocks)
        for feather in RR.FEATHERS:
            want, covered = RR.paste(PHOTOS, rows, cells, blocks, mode, RR.inv_ramp(rows, feather))
            got, buf = run_paste(ops, PHOTOS, rows, cells, blocks, mode, feather)
            same_photos(got, want, 'n %d mode %d blocks %d feather %g' % (n, mode, blocks, feather))
            # the padding between the photos, and every byte outside every box (the restatement leaves both alone)
            assert np.array_equal(buf, RR.pack(want)[0])
            for g, p, cov in zip(got, PHOTOS, covered):
                assert np.array_equal(g[~cov], p[~cov])
    if n == 65:                                             # the grid sized by the largest box itself (capped at 2^31 - 1 pixels)
        area = (rows[:, 3].astype(np.int64) - rows[:, 1]) * (rows[:, 4].astype(np.int64) - rows[:, 2])
        got, _buf = run_paste(ops, PHOTOS, rows, ref_cells(n, 8), 8, mode, 0.125, max_pixels=int(min(area.max(), 2 ** 31 - 1)))
        same_photos(got, RR.paste(PHOTOS, rows, ref_cells(n, 8), 8, mode, RR.inv_ramp(rows, 0.125))[0], 'the full grid')


# ----------------------------------------------------------------------------------------------------------------------------
# 3. the paste with the mask: exact, fail closed, and the weight bit for bit
# ----------------------------------------------------------------------------------------------------------------------------
def wild_hull(rows, seed=9):
    """hull_case with wild contents in rows that are not flagged: NaN, +-inf and 1e30 in some lines and inv_soft."""
    poses, edges, flags, isoft, special = RR.hull_case(rows)
    edges, isoft = edges.copy(), isoft.copy()
    plain = [b for b in range(len(rows)) if not flags[b] and b not in special]
    for k, b in enumerate(plain[2:10]):                                  # the first two stay ordinary hulls
        what = (np.nan, np.inf, -np.inf, 1e30, -1e30)[k % 5]
        if k < 5:
            edges[b, k % edges.shape[1], k % 3] = what
        else:
            isoft[b] = what
    return edges, isoft, flags, special, plain


@pytest.mark.parametrize('mode', [RR.PIXELATE, RR.SMOOTH])
def test_masked_paste_equals_the_restatement_and_fails_closed(ops, mode):
    n = 65
    rows = RR.case_rows(n)
    edges, isoft, flags, (nan_row, flat_row), plain = wild_hull(rows)
    assert flags[nan_row] & 1 and flags[flat_row] == 2 and len(plain) >= 10
    for blocks in (1, 7, 64):
        cells = ref_cells(n, blocks).copy()
        for b in range(n):                                               # wild bytes past every row's grid: they are never read
            _cell, gy, gx = RR.grid(rows[b], blocks)
            cells[b, gy * gx * 3:] = 0xA5
        for feather in RR.FEATHERS:
            want, covered = RR.paste(PHOTOS, rows, cells, blocks, mode, RR.inv_ramp(rows, feather), edges, isoft, flags)
            got, buf = run_paste(ops, PHOTOS, rows, cells, blocks, mode, feather, hull=(edges, isoft, flags))
            same_photos(got, want, 'masked mode %d blocks %d feather %g' % (mode, blocks, feather))
            assert np.array_equal(buf, RR.pack(want)[0])
    # fail closed: the flagged rows alone at feather 0 in the pixelate mode: every pixel of the box in the photo is its cell's mean
    if mode == RR.PIXELATE:
        for fr in (nan_row, flat_row):
            one = rows[fr:fr + 1]
            hull = (edges[fr:fr + 1], isoft[fr:fr + 1], flags[fr:fr + 1])
            got, _buf = run_paste(ops, PHOTOS, one, RR.cells_all(PHOTOS, one, 7), 7, mode, 0.0, hull=hull)
            box_is_its_means(got[one[0, 0]], PHOTOS[one[0, 0]], one[0], 7, 'flagged row %d' % fr)
            # with its flag cleared the same lines (0, 0, -inf) write nothing: the flag is what covers the box
            got, _buf = run_paste(ops, PHOTOS, one, RR.cells_all(PHOTOS, one, 7), 7, mode, 0.0, hull=(hull[0], hull[1], np.zeros(1, np.int32)))
            same_photos(got, PHOTOS, 'the flag cleared')


def test_hull_weight_path_is_hull_references_bit_for_bit(ops):
    """A pixelate run whose cells are 255 over a zero photo: the byte is rint(255 a), a = ramp * w with w from hull_reference."""
    rows = RR.case_rows(len(RR.ROWS))
    _poses, edges, flags, isoft, special = RR.hull_case(rows)
    zero = [np.zeros_like(p) for p in PHOTOS]
    checked = 0
    for b in range(len(rows)):
        row = rows[b].tolist()
        if flags[b] or b in special or not RR.active(row, 3) or row[3] - row[1] > 1000 or RR._box_pixels(row, *PHOTOS[row[0]].shape[:2]) is None:
            continue
        for feather in RR.FEATHERS:
            one = rows[b:b + 1]
            ramp = RR.inv_ramp(one, feather)
            got, _buf = run_paste(ops, zero, one, np.full((1, 8 * 8 * 3), 255, np.uint8), 8, RR.PIXELATE, feather,
                                  hull=(edges[b:b + 1], isoft[b:b + 1], np.zeros(1, np.int32)))
            H, W = row[3] - row[1], row[4] - row[2]
            w = HR.weight_f32(edges[b], isoft[b], H, W)
            r, c = np.arange(H), np.arange(W)
            a = (np.minimum(F32(1), (np.minimum(r, H - 1 - r).astype(F32) + F32(0.5)) * ramp[0, 0])[:, None] *
                 np.minimum(F32(1), (np.minimum(c, W - 1 - c).astype(F32) + F32(0.5)) * ramp[0, 1])[None, :]) * w
            want = np.rint(F32(255) * a).astype(np.uint8)
            rr, cc = RR._box_pixels(row, *PHOTOS[row[0]].shape[:2])
            assert np.array_equal(got[row[0]][rr, cc, 0], want[rr - row[1], cc - row[2]]), (b, feather)
            checked += int((w > 0).any() and (w < 1).any())
    assert checked >= 8


# ----------------------------------------------------------------------------------------------------------------------------
# 4. split invariance
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [RR.PIXELATE, RR.SMOOTH])
def test_rows_split_into_launches_give_the_bytes_of_one(ops, mode):
    n = len(RR.ROWS)
    rows = RR.case_rows(n)
    cells = ref_cells(n, 7)                                              # taken once, from the original
    edges, isoft, flags, _special, _plain = wild_hull(rows)
    for hull in (None, (edges, isoft, flags)):
        _photos, whole = run_paste(ops, PHOTOS, rows, cells, 7, mode, 0.125, hull=hull)
        for launches in ([(0, 3), (3, n)], [(i, i + 1) for i in range(n)]):
            _photos, parts = run_paste(ops, PHOTOS, rows, cells, 7, mode, 0.125, hull=hull, launches=launches)
            assert np.array_equal(parts, whole), (hull is not None, len(launches))


# ----------------------------------------------------------------------------------------------------------------------------
# 5. consequences (a) and (b) of the header, on the device
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', [RR.PIXELATE, RR.SMOOTH])
def test_consequences_a_and_b_hold_byte_for_byte(ops, mode):
    # (a) cell == 1: blocks >= max(H, W)
    rows = np.array([(0, 3, 4, 33, 50), (1, -5, 10, 40, 74), (1, 20, 30, 60, 70), (2, 0, 0, 1, 1)], np.int32)
    edges, flags = HR.hull_fit(np.random.RandomState(2).uniform(-0.8, 0.8, (4, 7, 2)).astype(F32), rows, np.full(4, 1.25, F32))
    for feather in RR.FEATHERS:
        for hull in (None, (edges, HR.inv_soft(rows, 0.1), flags)):
            cells = run_cells(ops, PHOTOS, rows, 64)
            got, buf = run_paste(ops, PHOTOS, rows, cells, 64, mode, feather, hull=hull)
            same_photos(got, PHOTOS, '(a) feather %g' % feather)
            assert np.array_equal(buf, RR.pack(PHOTOS)[0])
    # (b) flat photos: every row in the pixelate mode; in the smooth mode the rows every cell of which holds a pixel
    flat = [np.full((37, 53, 3), (200, 17, 255), np.uint8), np.full((64, 80, 3), 1, np.uint8), np.zeros((1, 1, 3), np.uint8)]
    for blocks in (1, 7):
        rows = RR.case_rows(len(RR.ROWS))
        if mode == RR.SMOOTH:
            rows = rows[[RR.full_grid(r, blocks, RR.SIZES) for r in rows]]
        assert len(rows) >= 7
        got, _buf = run_paste(ops, flat, rows, run_cells(ops, flat, rows, blocks), blocks, mode, 0.125)
        same_photos(got, flat, '(b) blocks %d' % blocks)


# ----------------------------------------------------------------------------------------------------------------------------
# 6. LandmarkDetector.redact
# ----------------------------------------------------------------------------------------------------------------------------
GROW = 16.0                      # the landmarks of a model with random weights lie within a pixel or two of each other: the largest
                                 # grow gives their hull an inside worth testing
SCENE_SIZES = [(150, 131), (120, 163)]
SCENE_BOXES = [(0, 10, 12, 100, 90), (1, 5, 20, 90, 101), (0, 60, 50, 160, 140), (1, 30, 80, 110, 150), (1, -10, -8, 50, 40)]
APART = [(0, 10, 12, 100, 90), (1, 5, 20, 90, 101), (1, 30, 110, 100, 160)]          # no two overlap


@pytest.fixture(scope='module')
def world(ops):
    cfg, model, eng, P, St = D.make_model(10, 128, 2)
    return dict(model=model, eng=eng, det=model.landmark_detector(128, max_batch=4),
                photos=[AR.smooth_photo(h, w, 40 + i) for i, (h, w) in enumerate(SCENE_SIZES)])


def host(t):
    return t.cpu().numpy()


def test_detector_redact_without_a_mask_runs_no_pose_program(ops, world):
    det, photos = world['det'], world['photos']
    rows = np.array(SCENE_BOXES, np.int32)
    for mode, code in (('pixelate', RR.PIXELATE), ('smooth', RR.SMOOTH)):
        for blocks, feather in ((8, 0.0), (5, 0.125)):
            (out, tr), calls = _count_calls(ops, lambda: det.redact(photos, SCENE_BOXES, mode=mode, blocks=blocks, feather=feather,
                                                                    return_transform=True))
            # n = 5 rows at max_batch 4: two buckets, two launches each, and nothing else: no crop, no pose program
            assert calls == ['imm_redact_cells_u8', 'imm_redact_u8'] * 2, calls
            cells = RR.cells_all(photos, rows, blocks)
            want, _cov = RR.paste(photos, rows, cells, blocks, code, RR.inv_ramp(rows, feather))
            assert all(o.is_cuda and o.dtype == torch.uint8 for o in out)
            same_photos([host(o) for o in out], want, 'redact %s blocks %d feather %g' % (mode, blocks, feather))
            assert np.array_equal(host(tr.cells), cells) and tr.mu is None and tr.hull_edges is None and tr.hull_flags is None
            assert tr.cell.tolist() == [RR.grid(r, blocks)[0] for r in rows] and tr.grid.tolist() == [list(RR.grid(r, blocks)[1:]) for r in rows]
            assert (tr.mode, tr.blocks) == (mode, blocks) and np.array_equal(tr.means(2), cells[2][:tr.grid[2].prod() * 3].reshape(*tr.grid[2], 3))
    # the defaults: pixelate, 8 blocks, the hard whole box: every box is its means where no later row lies over it
    out = det.redact(photos, APART)
    for row in APART:
        box_is_its_means(host(out[row[0]]), photos[row[0]], row, 8, 'the defaults')
    # two buckets give the bytes of one
    one = world['model'].landmark_detector(128, max_batch=8)
    lm = np.random.RandomState(6).uniform(-0.7, 0.7, (len(SCENE_BOXES), 10, 2)).astype(F32)
    for kw in (dict(mode='smooth', feather=0.125), dict(mode='pixelate', mask='hull', feather=0.125, landmarks=lm)):
        a, b = det.redact(photos, SCENE_BOXES, **kw), one.redact(photos, SCENE_BOXES, **kw)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), kw


def test_detector_redact_with_the_hull_mask(ops, world):
    det, photos = world['det'], world['photos']
    rows = np.array(SCENE_BOXES, np.int32)
    n = len(rows)
    det.redact(photos, SCENE_BOXES, mask='hull')                                                # (captures out of the way)
    for mode, code in (('pixelate', RR.PIXELATE), ('smooth', RR.SMOOTH)):
        (out, tr), calls = _count_calls(ops, lambda: det.redact(photos, SCENE_BOXES, mode=mode, blocks=6, mask='hull', grow=GROW,
                                                                mask_feather=0.2, feather=0.125, return_transform=True))
        assert [c for c in calls if c.startswith('imm_redact') or c == 'imm_hull_fit'] == ['imm_hull_fit', 'imm_redact_cells_u8', 'imm_redact_u8'] * 2
        assert calls.count('imm_resize_crop_u8') == 2
        mu = host(tr.mu)
        assert np.array_equal(mu, host(det.landmarks(photos, SCENE_BOXES))), 'the hull is fitted to the detector\'s landmarks'
        edges, flags = HR.hull_fit(mu, rows, np.full(n, GROW, F32))
        isoft = HR.inv_soft(rows, 0.2)
        assert np.array_equal(host(tr.hull_edges).view(np.uint32), edges.view(np.uint32)) and np.array_equal(host(tr.hull_flags), flags)
        assert np.array_equal(tr.inv_soft, isoft)
        cells = RR.cells_all(photos, rows, 6)
        want, covered = RR.paste(photos, rows, cells, 6, code, RR.inv_ramp(rows, 0.125), edges, isoft, flags)
        same_photos([host(o) for o in out], want, 'redact %s with the hull' % mode)
        print('\nREDACT hull %s: flags %s, pixels written %s of %s' % (mode, flags.tolist(), [int(c.sum()) for c in covered],
                                                                     [c.size for c in covered]))
        w = tr.weight(0)
        assert w.shape == (90, 78) and w.dtype == F32 and ((w > 0) == covered[0][10:100, 12:90])[:50, :38].all()
    # landmarks= : the pose program is skipped, and a row with a NaN is redacted over its whole box
    lm = np.random.RandomState(4).uniform(-0.7, 0.7, (len(APART), 10, 2)).astype(F32)
    lm[1, 4, 1] = np.nan
    (out, tr), calls = _count_calls(ops, lambda: det.redact(photos, APART, mask='hull', landmarks=lm, return_transform=True))
    assert calls == ['imm_hull_fit', 'imm_redact_cells_u8', 'imm_redact_u8'], calls
    assert [f & 1 for f in host(tr.hull_flags).tolist()] == [0, 1, 0] and host(tr.hull_flags)[0] == 0 == host(tr.hull_flags)[2]
    assert np.array_equal(host(tr.mu).view(np.uint32), lm.view(np.uint32))
    box_is_its_means(host(out[1]), photos[1], APART[1], 8, 'the NaN row')
    row = APART[0]
    inside = host(out[0])[row[1]:row[3], row[2]:row[4]]
    assert (inside == photos[0][row[1]:row[3], row[2]:row[4]]).all(axis=2).any(), 'an ordinary row leaves the pixels outside its hull'
    assert (tr.weight(1) == 1).all() and (tr.weight(0) == 0).any()


# ----------------------------------------------------------------------------------------------------------------------------
# 7. LandmarkDetector.redact_clip
# ----------------------------------------------------------------------------------------------------------------------------
FACES = [(20, 24, 110, 100), (40, 120, 120, 190)]


def clip_frames(T=5):
    big = AR.smooth_photo(170, 230, 77)
    return [np.ascontiguousarray(big[8 - 2 * t:8 - 2 * t + 150, 3 * t:3 * t + 210]) for t in range(T)]


@pytest.mark.parametrize('mask', [None, 'hull'])
def test_redact_clip_equals_redact_per_frame(ops, world, mask):
    from imm_amd.redaction import ClipRedaction
    det, frames = world['det'], clip_frames()
    T, Fn = len(frames), len(FACES)
    kw = dict(mode='smooth' if mask else 'pixelate', blocks=6, mask=mask, grow=GROW, mask_feather=0.15, feather=0.125 if mask else 0.0)
    det.redact_clip(frames[:2], FACES, **kw)                                                    # (captures and allocations out of the way)
    cr, calls = _count_calls(ops, lambda: det.redact_clip(frames, FACES, chunk_frames=3, **kw))
    assert isinstance(cr, ClipRedaction) and len(cr) == T and len(cr.frames) == T and tuple(cr.own.shape) == (T, Fn, 10, 2)
    assert (cr.hull_flags is not None) == (mask == 'hull') and calls.count('imm_hull_fit') == (T if mask else 0)
    assert calls.count('imm_redact_cells_u8') == T == calls.count('imm_redact_u8') == calls.count('imm_clip_rows')
    boxes, own = host(cr.track.boxes), host(cr.own)
    print('\nREDACT CLIP mask=%s: %d lost, boxes of the last frame %s' % (mask, int(host(cr.track.lost).sum()), boxes[-1].tolist()))
    for t in range(T):
        rows = np.concatenate([np.zeros((Fn, 1), np.int32), boxes[t]], axis=1)
        want = det.redact([frames[t]], rows.tolist(), landmarks=torch.from_numpy(own[t]), **kw)[0]
        assert cr.frames[t].dtype == torch.uint8 and tuple(cr.frames[t].shape) == frames[t].shape
        assert torch.equal(cr.frames[t], want), 'frame %d' % t
        changed = int((host(cr.frames[t]) != frames[t]).any(axis=2).sum())
        print('frame %d: %d pixels changed' % (t, changed))
        assert changed or mask == 'hull'          # (a small hull over a smooth photo may blur to the same bytes)
        if mask is None:
            for row in rows:
                box_is_its_means(host(cr.frames[t]), frames[t], row, 6, 'frame %d' % t)


@pytest.mark.parametrize('mask', [None, 'hull'])
def test_a_face_the_gate_finds_unsure_is_covered_whole(ops, world, mask):
    """gate = QualityGate(max_spread=1e-30), the nearest the gate allows to 0 (a threshold must be > 0; no spread of a soft-argmax is
    that small): every face is unsure on every frame, and on EVERY frame every box is covered whole.  The tracker keeps the first
    frame's faces (the caller vouches for the first boxes) and loses them on every later frame; a lost face keeps its box.  On the
    first frame the faces have finite landmarks and a hull of their own: there it is the gate's verdict, folded into hull_flags as
    bit 2, that covers the box."""
    from imm_amd.quality import QualityGate
    from imm_amd.redaction import FLAG_UNSURE
    det, frames = world['det'], clip_frames()
    T, Fn = len(frames), len(FACES)
    kw = dict(mode='pixelate', blocks=6, mask=mask, grow=GROW, feather=0.0)
    cr = det.redact_clip(frames, FACES, gate=QualityGate(max_spread=1e-30), **kw)
    assert host(cr.track.unsure).all() and host(cr.track.lost)[1:].all() and not host(cr.track.lost)[0].any()
    boxes = host(cr.track.boxes)
    if mask == 'hull':
        hf = host(cr.hull_flags)
        assert (hf & FLAG_UNSURE).all() and (hf[0] == FLAG_UNSURE).all() and (hf[1:] & 1).all()
        assert np.isfinite(host(cr.own)[0]).all() and np.isnan(host(cr.own)[1:]).all()
    for t in range(T):
        for f in range(Fn):
            box_is_its_means(host(cr.frames[t]), frames[t], [0] + boxes[t, f].tolist(), 6, 'frame %d face %d' % (t, f))
    assert (boxes[2:] == boxes[1]).all(), 'a lost face keeps the box the tracker\'s unchanged state gives it'
    if mask == 'hull':
        # the control: without a gate the same first frame wears its hulls only (pixels of the box keep their bytes), no bit 2 is set
        plain = det.redact_clip(frames[:2], FACES, **kw)
        assert not (host(plain.hull_flags) & FLAG_UNSURE).any() and not host(plain.hull_flags)[0].any()
        y0, x0, y1, x1 = FACES[0]
        assert (host(plain.frames[0])[y0:y1, x0:x1] == frames[0][y0:y1, x0:x1]).all(axis=2).any()
        assert not torch.equal(plain.frames[0], cr.frames[0])


# ----------------------------------------------------------------------------------------------------------------------------
# 8. the script
# ----------------------------------------------------------------------------------------------------------------------------
def test_detect_script_redacts(ops, world, tmp_path, capsys):
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
    rows = [(files[0], 20, 10, 180, 150), (files[2], -10, 30, 120, 170), (files[0], 100, 60, 215, 175)]
    boxes = str(tmp_path / 'faces.csv')
    with open(boxes, 'w') as f:
        f.write('file,y0,x0,y1,x1\n' + ''.join('%s,%d,%d,%d,%d\n' % r for r in rows))
    script = os.path.join(ROOT, 'scripts', 'detect.py')
    common = ['--configs', conf, '--checkpoint', ckpt, '--images-dir', imdir, '--batch-size', '4', '--boxes', boxes]
    det = LandmarkDetector.from_checkpoint(load_configs([conf]).model, ckpt, image_size=128, max_batch=4, device=DEV)
    photos = [pixels[f] for f in files]
    api_rows = [(files.index(r[0]),) + r[1:] for r in rows]
    for extra, kw in ((['--redact', 'pixelate'], dict(mode='pixelate')),
                      (['--redact', 'smooth', '--blocks', '5', '--mask', 'hull', '--grow', '1.1', '--mask-feather', '0.2', '--feather', '0.125'],
                       dict(mode='smooth', blocks=5, mask='hull', grow=1.1, mask_feather=0.2, feather=0.125))):
        out_dir = str(tmp_path / ('out%d' % len(extra)))
        D._run_script(script, common + extra + ['--out-dir', out_dir])
        assert '3 faces redacted in 4 images' in capsys.readouterr().out
        want = det.redact(photos, api_rows, **kw)
        for f, w, p in zip(files, want, photos):
            png = np.asarray(Image.open(os.path.join(out_dir, os.path.splitext(f)[0] + '.png')))
            assert np.array_equal(png, host(w)), f
        assert (host(want[0]) != photos[0]).any() and np.array_equal(host(want[1]), photos[1])
    with pytest.raises(ValueError, match='--out-dir'):
        D._run_script(script, common + ['--redact', 'pixelate'])
    for extra in (['--out-dir', str(tmp_path / 'no')], ['--blocks', '4'], ['--mask', 'hull'], ['--grow', '1.5'], ['--mask-feather', '0.3'],
                  ['--feather', '0.1']):
        with pytest.raises(ValueError, match='go with --redact'):
            D._run_script(script, common + extra)
    # --track --redact: the folder is one clip, the faces of its first frame are followed and redacted on every frame
    first = str(tmp_path / 'first.csv')
    faces = [(30, 20, 170, 140), (110, 70, 210, 170)]
    with open(first, 'w') as f:
        f.write(''.join('%s,%d,%d,%d,%d\n' % ((files[0],) + r) for r in faces))
    out_dir = str(tmp_path / 'clip')
    D._run_script(script, [a if a != boxes else first for a in common] + ['--track', '--redact', 'smooth', '--blocks', '5', '--mask', 'hull',
                                                                        '--out-dir', out_dir])
    assert '4 frames, 2 faces redacted' in capsys.readouterr().out
    cr = det.redact_clip(photos, [list(r) for r in faces], mode='smooth', blocks=5, mask='hull')
    for f, w in zip(files, cr.frames):
        assert np.array_equal(np.asarray(Image.open(os.path.join(out_dir, os.path.splitext(f)[0] + '.png'))), host(w)), f
    with pytest.raises(ValueError, match='blocks'):
        D._run_script(script, common + ['--redact', 'pixelate', '--blocks', '65', '--out-dir', str(tmp_path / 'no')])
