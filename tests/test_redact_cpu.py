"""Redaction, host side (no GPU): the ABI of imm_redact_cells_u8 / imm_redact_u8 and their argument validation, the wrapper and
plan_redact refusals, hand-derived known answers of the cell rule, the consequences (a)-(d) of include/imm_redact.h on the restatement
(tests/redact_reference.py), its hull weight against hull_reference's, the fail-closed rule, and the f32 restatement against the f64
one on the GPU test's cases."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_reference as HR                                                 # noqa: E402
import redact_reference as RR                                               # noqa: E402

from imm_amd import redaction as RD                                         # noqa: E402  (imports without a GPU)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAMES = ['imm_redact_cells_u8', 'imm_redact_u8']


# ----------------------------------------------------------------------------------------------------------------------------
# ABI and validation
# ----------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_redact_entry_points():
    from imm_amd import _lib as L
    assert L.ABI_VERSION >= 37
    assert L.symbols('imm_redact.h') == NAMES
    header = open(os.path.join(ROOT, 'include', 'imm_redact.h')).read()
    for text in ('THE RULE', 'Cells (imm_redact_cells_u8)', 'Paste (imm_redact_u8)', 'Fail closed', 'rounded separately', 'Consequences'):
        assert text in header, text
    assert 'typedef struct' not in header
    src = open(os.path.join(ROOT, 'imm_amd', 'csrc', 'redact.hip')).read()
    assert 'fp contract(off)' in src and 'asm' not in src.lower() and 'atomic' not in src.lower().replace('no atomics', '')
    assert 'redact_hull_weight' in src and 'RedactPolicy<HULL>' in src and 'paste_rows(' in src
    assert RD.MODES == {'pixelate': 0, 'smooth': 1} and RD.MAX_BLOCKS == 64


def test_redact_entry_points_validate_their_arguments_without_a_device():
    from imm_amd import _lib as L
    lib = L.load()
    one, two, three = C.c_void_p(16), C.c_void_p(32), C.c_void_p(48)     # non-null pointers that are never read: validation comes first
    #       src offs hw n_img boxes blocks n cells stream
    good = [one, one, one, 2, one, 8, 3, two, None]
    bad_args = [(i, None) for i in (0, 1, 2, 4, 7)] + [(3, 0), (5, 0), (5, 65), (5, -1), (6, 0), (6, -1), (6, 65536)]
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert lib.imm_redact_cells_u8(*args) == -1, (i, bad)
        assert b'redact_cells_u8' in lib.imm_last_error()
    #       dst offs hw n_img boxes links ramp cells blocks mode edges soft flags K  n  pixels stream
    good = [one, one, one, 2, one, one, one, two, 8, 0, three, three, three, 10, 3, 100, None]
    bad_args = [(i, None) for i in (0, 1, 2, 4, 5, 6, 7)]                   # every pointer NULL in turn ...
    bad_args += [(i, None) for i in (10, 11, 12)]                           # ... which for the nullable trio is "given in part"
    bad_args += [(7, one), (3, 0), (8, 0), (8, 65), (9, 2), (9, -1), (13, 0), (13, 81), (14, 0), (14, 65536), (15, 0), (15, -5)]
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert lib.imm_redact_u8(*args) == -1, (i, bad)
        assert b'redact_u8' in lib.imm_last_error() and b'redact_cells_u8' not in lib.imm_last_error()
    # two of the trio absent is "in part" as well; without the trio K is not read (the refusal below is the one of n)
    for pair in ((10, 11), (10, 12), (11, 12)):
        args = list(good)
        for i in pair:
            args[i] = None
        assert lib.imm_redact_u8(*args) == -1 and b'all NULL or all given' in lib.imm_last_error()
    args = list(good)
    args[10] = args[11] = args[12] = None
    args[13], args[14] = 0, 0
    assert lib.imm_redact_u8(*args) == -1 and b'rows' in lib.imm_last_error()


def test_wrapper_refusals_come_before_any_device_call():
    from imm_amd import ops
    z = lambda *sh, **kw: torch.zeros(*sh, **kw)           # host tensors: a wrapper that got as far as the library would fault
    n, K, nb = 2, 10, 8
    buf, offs, hw = z(64, dtype=torch.uint8), z(1, dtype=torch.int64), z(1, 2, dtype=torch.int32)
    boxes, cells = z(n, 5, dtype=torch.int32), z(n, nb * nb * 3, dtype=torch.uint8)
    for kw, match in ((dict(boxes=z(n, 4, dtype=torch.int32)), 'boxes'), (dict(boxes=boxes.long()), 'boxes'), (dict(boxes=boxes[:0]), 'rows'),
                      (dict(blocks=0), 'blocks'), (dict(blocks=65), 'blocks'), (dict(blocks=2.5), 'blocks'), (dict(blocks=True), 'blocks'),
                      (dict(cells=z(n, nb * nb, dtype=torch.uint8)), 'cells'), (dict(cells=cells.int()), 'cells'),
                      (dict(cells=buf[:0].view(0, 3)), 'cells'), (dict(src=buf.float()), 'photos'), (dict(hw=z(0, 2, dtype=torch.int32)), 'hw'),
                      (dict(offsets=z(2, dtype=torch.int64)), 'offsets'), (dict(src=cells.view(-1), cells=cells), 'overlaps')):
        args = dict(src=buf, offsets=offs, hw=hw, boxes=boxes, blocks=nb, cells=cells)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.redact_cells_u8(**args)
    links, ramp = z(n, 2, dtype=torch.int32), z(n, 2)
    edges, soft, flags = z(n, K, 3), z(n), z(n, dtype=torch.int32)
    for kw, match in ((dict(mode=2), 'mode'), (dict(mode='blur'), 'mode'), (dict(links=z(n, 2)), 'links'), (dict(inv_ramp=z(n)), 'inv_ramp'),
                      (dict(max_box_pixels=0), 'max_box_pixels'), (dict(edges=None), 'come together'), (dict(inv_soft=None), 'come together'),
                      (dict(hull_flags=None), 'come together'), (dict(edges=z(n, 81, 3)), 'edges'), (dict(edges=z(n, K, 2)), 'edges'),
                      (dict(inv_soft=soft.double()), 'inv_soft'), (dict(hull_flags=flags.long()), 'hull_flags'), (dict(blocks=65), 'blocks'),
                      (dict(dst=cells.view(-1)), 'overlaps'), (dict(dst=boxes.view(torch.uint8).view(-1)), 'boxes overlaps'),
                      (dict(dst=hw.view(torch.uint8).view(-1)), 'hw overlaps')):
        args = dict(dst=buf, offsets=offs, hw=hw, boxes=boxes, links=links, inv_ramp=ramp, cells=cells, blocks=nb, mode=0, max_box_pixels=9,
                    edges=edges, inv_soft=soft, hull_flags=flags)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.redact_u8(**args)


# ----------------------------------------------------------------------------------------------------------------------------
# plan_redact
# ----------------------------------------------------------------------------------------------------------------------------
def test_plan_redact_refusals_and_its_acceptance_of_landmarks_that_are_not_finite():
    photos = [np.zeros((40, 50, 3), np.uint8), np.zeros((30, 30), np.uint8)]
    K = 10
    plan = RD.plan_redact(photos, None, K)
    assert set(vars(plan)) == set(RD.RedactPlan.FIELDS)
    assert (plan.mode, plan.blocks, plan.feather, plan.mask, plan.landmarks) == ('pixelate', 8, 0.0, None, None)
    assert plan.rows.tolist() == [[0, 0, 0, 40, 50], [1, 0, 0, 30, 30]] and plan.rows.dtype == np.int32
    assert plan.grow.tolist() == [1.25, 1.25] and np.array_equal(plan.inv_soft, HR.inv_soft(plan.rows, 0.1))
    for kw, match in ((dict(mode='blur'), 'mode'), (dict(mode=0), 'mode'), (dict(mode=None), 'mode'), (dict(blocks=0), 'blocks'),
                      (dict(blocks=65), 'blocks'), (dict(blocks=8.0), 'blocks'), (dict(blocks=True), 'blocks'), (dict(blocks='8'), 'blocks'),
                      (dict(feather=-0.1), 'feather'), (dict(feather=0.6), 'feather'), (dict(feather=float('nan')), 'feather'),
                      (dict(mask='box'), 'mask'), (dict(mask=True), 'mask'), (dict(grow=0.0), 'grow'), (dict(mask_feather=1.5), 'mask_feather'),
                      (dict(landmarks=np.zeros((2, K))), 'landmarks'), (dict(landmarks=np.zeros((3, K, 2))), 'landmarks'),
                      (dict(landmarks=np.zeros((2, K + 1, 2))), 'landmarks'), (dict(boxes=[(0, 5, 5, 5, 9)]), 'empty'),
                      (dict(boxes=[(2, 0, 0, 4, 4)]), 'names image')):
        args = dict(photos=photos, boxes=None, K=K)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            RD.plan_redact(**args)
    with pytest.raises(ValueError):
        RD.plan_redact(np.zeros((2, 8, 8, 3), np.uint8), None, K)
    lm = np.zeros((2, K, 2), np.float32)
    lm[1, 3, 0], lm[0, 0, 1] = np.nan, np.inf
    plan = RD.plan_redact(photos, None, K, mode='smooth', blocks=64, mask='hull', landmarks=lm)          # not refused: redacted whole
    assert plan.landmarks.dtype == torch.float32 and bool(torch.isnan(plan.landmarks[1, 3, 0])) and plan.mask == 'hull'
    clip = RD.plan_redact_clip([photos[0]] * 3, [(2, 3, 30, 40)], K, blocks=4, mask='hull')
    assert len(clip.frames) == 3 and clip.rows.tolist() == [[0, 2, 3, 30, 40]] and clip.redact.blocks == 4 and clip.redact.mask == 'hull'
    with pytest.raises(ValueError, match='blocks'):
        RD.plan_redact_clip([photos[0]] * 3, [(2, 3, 30, 40)], K, blocks=0)


def test_cell_size_and_grid_shape_are_the_restatements():
    for H, W, blocks in ((4, 6, 2), (1, 1, 64), (5, 90, 8), (100000, 100000, 64), (37, 53, 7), (64, 64, 64), (65, 3, 64), (0, 5, 3), (5, -1, 3)):
        cell, gy, gx = RR.grid((0, 0, 0, H, W), blocks)
        assert RD.cell_size(H, W, blocks) == cell and RD.grid_shape(H, W, blocks) == (gy, gx)
        assert gy <= blocks and gx <= blocks
        if cell:
            assert (gy - 1) * cell < H <= gy * cell and (gx - 1) * cell < W <= gx * cell


# ----------------------------------------------------------------------------------------------------------------------------
# known answers, by hand
# ----------------------------------------------------------------------------------------------------------------------------
def ramp_photo(h, w):
    """photo[r, c] = (10 r + c, r, c)."""
    r, c = np.mgrid[0:h, 0:w]
    return np.stack([10 * r + c, r, c], axis=2).astype(np.uint8)


def test_cells_of_a_4_by_6_box_at_two_blocks():
    photo = ramp_photo(8, 10)
    row = (0, 1, 2, 5, 8)                                   # H = 4, W = 6: cell = 3, grid 2 x 2, the second cell row is one pixel high
    assert RR.grid(row, 2) == (3, 2, 2)
    got = RR.cells(photo, row, 2).reshape(2, 2, 3)
    # cell (0, 0): rows 1..3, columns 2..4: mean of 10 r + c = 20 + 3 = 23; (0, 1): columns 5..7: 26
    # cell (1, 0): row 4 alone: 40 + 3 = 43; (1, 1): 46
    assert got.tolist() == [[[23, 2, 3], [26, 2, 6]], [[43, 4, 3], [46, 4, 6]]]
    # a half that rounds UP: the box rows 1..2 (H = 2) by one column at blocks = 1: mean of r is 1.5 -> 2, of 10 r + c = (12 + 22) / 2 = 17
    assert RR.cells(photo, (0, 1, 2, 3, 3), 1).tolist() == [17, 2, 2]
    # and .5 in the first channel: rows 1..2, columns 2..3: (12 + 13 + 22 + 23) / 4 = 17.5 -> 18; r: 1.5 -> 2; c: 2.5 -> 3
    assert RR.cells(photo, (0, 1, 2, 3, 4), 1).tolist() == [18, 2, 3]
    # the rest of a slice is zeros
    wide = RR.cells(photo, row, 5)                          # cell 2: grid 2 x 3
    assert RR.grid(row, 5) == (2, 2, 3) and wide.shape == (75,) and not wide[18:].any()
    assert wide[:18].reshape(2, 3, 3)[1, 2].tolist() == [42, 4, 7]       # photo rows 3..4, columns 6..7: (36 + 37 + 46 + 47) / 4 = 41.5 -> 42


def test_cells_at_the_photo_edge_and_outside_it():
    photo = ramp_photo(8, 10)
    # blocks = 1 over a box that reaches 2 rows above and 2 columns left of the photo: only the 2 x 2 pixels in the photo count
    assert RR.cells(photo, (0, -2, -2, 2, 2), 1).tolist() == [6, 1, 1]          # (0 + 1 + 10 + 11) / 4 = 5.5 -> 6; 0.5 -> 1; 0.5 -> 1
    # blocks = 2: cell (0, 0), (0, 1) and (1, 0) lie wholly outside the photo: (0, 0, 0); cell (1, 1) is the 2 x 2 pixels
    got = RR.cells(photo, (0, -2, -2, 2, 2), 2).reshape(2, 2, 3)
    assert got.tolist() == [[[0, 0, 0], [0, 0, 0]], [[0, 0, 0], [6, 1, 1]]]
    # a cell cut by the bottom edge: the box rows 6..9 of an 8-row photo, blocks = 1: rows 6 and 7 only
    assert RR.cells(photo, (0, 6, 0, 10, 1), 1).tolist() == [65, 7, 0]          # (60 + 70) / 2 = 65; 6.5 -> 7
    # a box wholly outside, an empty one, an inverted one, no photo: zeros
    for row, ph in (((0, 20, 20, 30, 30), photo), ((0, 3, 3, 3, 6), photo), ((0, 5, 5, 2, 2), photo), ((7, 0, 0, 4, 4), None)):
        assert not RR.cells(ph, row, 3).any()
    # blocks = 1 (d): the box's own mean
    box = photo[2:7, 1:9].reshape(-1, 3).astype(np.int64)
    assert RR.cells(photo, (0, 2, 1, 7, 9), 1).tolist() == [(2 * int(s) + 40) // 80 for s in box.sum(axis=0)]


# ----------------------------------------------------------------------------------------------------------------------------
# the consequences of the header, on the restatement
# ----------------------------------------------------------------------------------------------------------------------------
def _run(photos, rows, blocks, mode, feather, dtype=np.float32, hull=None):
    cb = RR.cells_all(photos, rows, blocks)
    kw = {} if hull is None else dict(edges=hull[0], isoft=hull[1], hull_flags=hull[2])
    return RR.paste(photos, rows, cb, blocks, mode, RR.inv_ramp(rows, feather), dtype=dtype, **kw)


@pytest.mark.parametrize('mode', (RR.PIXELATE, RR.SMOOTH))
def test_consequence_a_cell_one_returns_the_photo(mode):
    photos = RR.photos_of()
    rows = np.array([(0, 3, 4, 33, 50), (1, -5, 10, 40, 74)], np.int32)          # max(H, W) = 46 and 64 <= blocks
    for feather in RR.FEATHERS:
        out, covered = _run(photos, rows, 64, mode, feather)
        assert all(np.array_equal(a, b) for a, b in zip(out, photos)) and covered[0].any()


FLAT = [np.full((37, 53, 3), (200, 17, 255), np.uint8), np.full((64, 80, 3), 1, np.uint8), np.zeros((1, 1, 3), np.uint8)]


def flat_rows(mode, blocks):
    """The rows of consequence (b): all of them in the pixelate mode; in the smooth mode those every cell of which holds a pixel (a
    cell wholly outside the photo has the mean 0, which the smooth mode's taps mix in: the header says so)."""
    rows = RR.case_rows(len(RR.ROWS))
    if mode == RR.SMOOTH:
        rows = rows[[RR.full_grid(r, blocks, RR.SIZES) for r in rows]]
    return rows


@pytest.mark.parametrize('mode', (RR.PIXELATE, RR.SMOOTH))
def test_consequence_b_a_flat_photo_comes_back(mode):
    for blocks in (1, 7):
        rows = flat_rows(mode, blocks)
        assert len(rows) >= 7 and any(r[1] < 0 or r[2] < 0 for r in rows)          # a box cut by the photo's edge is among them
        out, _cov = _run(FLAT, rows, blocks, mode, 0.125)
        assert all(np.array_equal(a, b) for a, b in zip(out, FLAT))
    # and what the header says of the smooth mode next to an empty cell: the pixels come out darker, never brighter
    row = np.array([(0, -20, 5, 20, 45)], np.int32)                     # blocks = 2: the upper cells lie outside the photo
    assert not RR.full_grid(row[0], 2, RR.SIZES)
    out, _cov = _run(FLAT, row, 2, RR.SMOOTH, 0.0)
    assert (out[0] <= FLAT[0]).all() and (out[0] < FLAT[0]).any()
    out, _cov = _run(FLAT, row, 2, RR.PIXELATE, 0.0)
    assert np.array_equal(out[0], FLAT[0])


def test_consequences_c_and_d_the_byte_is_the_cell_mean():
    photos = RR.photos_of()
    row = (1, 10, -4, 47, 60)
    rows = np.array([row], np.int32)
    for blocks in (1, 7):
        out, covered = _run(photos, rows, blocks, RR.PIXELATE, 0.0)
        cell, gy, gx = RR.grid(row, blocks)
        means = RR.cells(photos[1], row, blocks)[:gy * gx * 3].reshape(gy, gx, 3)
        r, c = np.nonzero(covered[1])
        assert len(r) == 37 * 60 and np.array_equal(out[1][r, c], means[(r - 10) // cell, (c + 4) // cell])
        if blocks == 1:                                     # (d): the box filled with its own mean
            assert len(np.unique(out[1][r, c], axis=0)) == 1
        assert np.array_equal(out[1][~covered[1]], photos[1][~covered[1]])


def test_the_restatements_weight_is_hull_references_and_a_flagged_row_covers_its_box():
    photos = RR.photos_of()
    rows = RR.case_rows(len(RR.ROWS))
    poses, edges, flags, isoft, (nan_row, flat_row) = RR.hull_case(rows)
    assert flags[nan_row] & 1 and flags[flat_row] & 2
    # the weight path: cells of 255 over a zero photo in the pixelate mode give the byte rint(255 a)
    zero = [np.zeros_like(p) for p in photos]
    b = 4
    row = rows[b].tolist()
    one = np.array([row], np.int32)
    cb = np.full((1, 8 * 8 * 3), 255, np.uint8)
    ramp = RR.inv_ramp(one, 0.125)
    out, _cov = RR.paste(zero, one, cb, 8, RR.PIXELATE, ramp, edges[b:b + 1], isoft[b:b + 1], np.zeros(1, np.int32))
    H, W = row[3] - row[1], row[4] - row[2]
    w = HR.weight_f32(edges[b], isoft[b], H, W)
    r, c = np.arange(H), np.arange(W)
    a = (np.minimum(F32(1), (np.minimum(r, H - 1 - r).astype(F32) + F32(0.5)) * ramp[0, 0])[:, None] *
         np.minimum(F32(1), (np.minimum(c, W - 1 - c).astype(F32) + F32(0.5)) * ramp[0, 1])[None, :]) * w
    want = np.rint(F32(255) * a).astype(np.uint8)
    assert (w > 0).any() and (w == 0).any() and (w == 1).any()
    rr, cc = np.mgrid[0:H, 0:W]
    assert np.array_equal(RR.weight_at(edges[b], isoft[b], rr, cc), w)
    assert np.array_equal(RR.weight_at(edges[b], isoft[b], rr, cc, wide=True), HR.weight_f64(edges[b], isoft[b], H, W))
    assert np.array_equal(out[row[0]][row[1]:row[3], row[2]:row[4], 0], want)
    # PhotoRedaction.weight is the same map
    tr = RD.PhotoRedaction(one, cb, 'pixelate', 8, 0.125, hull_edges=edges[b:b + 1], hull_flags=np.zeros(1, np.int32), inv_soft=isoft[b:b + 1])
    assert np.array_equal(tr.weight(0), a) and tr.cell.tolist() == [RR.grid(row, 8)[0]] and tr.grid.tolist() == [list(RR.grid(row, 8)[1:])]
    # fail closed: at feather 0 every pixel of a flagged row's box that lies in the photo is its cell mean
    for fr in (nan_row, flat_row):
        one = rows[fr:fr + 1]
        row = one[0].tolist()
        out, covered = _run(photos, one, 7, RR.PIXELATE, 0.0, hull=(edges[fr:fr + 1], isoft[fr:fr + 1], flags[fr:fr + 1]))
        cell, gy, gx = RR.grid(row, 7)
        means = RR.cells(photos[row[0]], row, 7)[:gy * gx * 3].reshape(gy, gx, 3)
        r, c = RR._box_pixels(row, *photos[row[0]].shape[:2])
        assert covered[row[0]][r, c].all() and np.array_equal(out[row[0]][r, c], means[(r - row[1]) // cell, (c - row[2]) // cell])
        # the same row with its flag cleared writes nothing: its lines are (0, 0, -inf)
        out, covered = _run(photos, one, 7, RR.PIXELATE, 0.0, hull=(edges[fr:fr + 1], isoft[fr:fr + 1], np.zeros(1, np.int32)))
        assert not covered[row[0]].any() and np.array_equal(out[row[0]], photos[row[0]])


@pytest.mark.parametrize('mode', (RR.PIXELATE, RR.SMOOTH))
@pytest.mark.parametrize('masked', (False, True))
def test_the_f32_restatement_stays_within_one_of_the_f64_one(mode, masked):
    """No byte differs by more than 1, and at most 1 % of the bytes differ, on the GPU test's cases."""
    photos = RR.photos_of()
    rows = RR.case_rows(65)
    hull = None
    if masked:
        _poses, edges, flags, isoft, _rows = RR.hull_case(rows)
        hull = (edges, isoft, flags)
    for blocks in RR.BLOCKS:
        for feather in RR.FEATHERS:
            a, _ = _run(photos, rows, blocks, mode, feather, np.float32, hull)
            b, _ = _run(photos, rows, blocks, mode, feather, np.float64, hull)
            diff = np.concatenate([np.abs(x.astype(np.int16) - y).reshape(-1) for x, y in zip(a, b)])
            print('mode %d masked %d blocks %d feather %g: max %d, %.4f %% differ' % (mode, masked, blocks, feather, diff.max(),
                                                                                    100.0 * (diff > 0).mean()))
            assert diff.max() <= 1 and (diff > 0).mean() <= 0.01
