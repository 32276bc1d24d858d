"""Annotation without a GPU: the ABI table, plan_annotate's refusals, the style tables, the script's refusals, and the properties of
the rule of include/imm_annotate.h on the numpy restatement (tests/annotate_reference.py) itself."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import annotate_reference as AN                   # noqa: E402
import hull_reference as HR                       # noqa: E402
import test_detector_gpu as D                     # noqa: E402  (_run_script)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
PHOTOS = AN.photos_of()


def test_abi_38_and_the_header_in_the_table():
    from imm_amd import _lib as L
    assert L.ABI_VERSION >= 38
    assert 'imm_annotate.h' in L.ABI and L.symbols('imm_annotate.h') == ['imm_annotate_points', 'imm_annotate_u8']
    assert list(L.ABI).index('imm_annotate.h') == list(L.ABI).index('imm_redact.h') + 1
    assert len(L.signature('imm_annotate_u8')[1]) == 23 and len(L.signature('imm_annotate_points')[1]) == 6
    text = open(os.path.join(ROOT, 'include', 'imm_annotate.h')).read()
    assert 'THE RULE' in text and 'int imm_annotate_points(' in text and 'int imm_annotate_u8(' in text


def test_annotation_imports_without_a_gpu_and_its_tables_are_the_projects():
    from imm_amd import annotation as A
    from imm_amd.utils import plot_landmarks as PL
    st = A.mark_styles(57)
    assert st.shape == (57, 4) and st.dtype == np.uint8
    for k in range(56):
        colour, marker = PL.get_marker_style(k)
        assert tuple(st[k, :3]) == tuple(colour) and PL.MARKERS[st[k, 3]] == marker == AN.SHAPES[st[k, 3]]
    assert np.array_equal(st[56], st[0]), 'past 56 the table starts again'
    assert np.array_equal(st, AN.mark_styles(57))
    assert np.array_equal(A.STATUS_PALETTE, AN.PALETTE) and A.STATUS_PALETTE.shape == (4, 3)
    bits = np.array([[[(int(v) >> (4 - c)) & 1 for c in range(5)] for v in d] for d in A.FONT], bool)
    assert np.array_equal(bits, AN.FONT_BITS), 'the font of the module is the font of the restatement'
    header = open(os.path.join(ROOT, 'include', 'imm_annotate.h')).read()
    for d in range(10):
        assert '%d: %s' % (d, ' '.join('%02X' % v for v in A.FONT[d])) in header, 'digit %d of the header' % d
    gs = A.group_styles(2.5, 4, 0.5)
    assert gs.shape == (4, 4) and gs.dtype == F32 and gs[3, 0] == F32(2.5) and gs[3, 1] == F32(0.2) and gs[3, 3] == F32(0.5)
    assert (gs[:3, 3] < 0.5).all() and (np.diff(gs[:3, 3]) > 0).all() and (gs[:, 2] >= 0.5).all()
    assert np.array_equal(gs, AN.group_styles(2.5, 4, 0.5))
    assert A.default_pad(2.5) == 5 and A.default_pad(6.0) == 8
    assert A.grid_pixels(np.array([(0, 0, 0, 10, 20), (0, 5, 5, 5, 5)]), 3) == 16 * 26
    assert A.draw_bits(('points', 'box')) == 3 and A.draw_bits(()) == 0 and A.draw_bits('hull,label') == 12


def test_plan_annotate_refuses_every_bad_argument_by_name():
    from imm_amd import annotation as A
    photos = [np.zeros((20, 30, 3), np.uint8)]
    boxes = [(0, 2, 3, 12, 13), (0, 4, 4, 18, 28)]
    ok = A.plan_annotate(photos, boxes, 10, draw=('points', 'box', 'hull', 'label'))
    assert ok.bits == 15 and ok.pad == 5 and ok.labels.tolist() == [0, 1] and ok.status is None and ok.group_style.shape == (1, 4)
    assert ok.max_pixels == (14 + 10) * (24 + 10) and ok.mark_style.shape == (10, 4)
    assert A.plan_annotate(photos, boxes, 10).labels is None
    for kw, word in ((dict(draw=('points', 'circle')), 'draw'), (dict(draw=3), 'draw'), (dict(size=0.0), 'size'), (dict(size=32.5), 'size'),
                     (dict(size=float('nan')), 'size'), (dict(thickness=0), 'thickness'), (dict(thickness=17), 'thickness'),
                     (dict(thickness=1.5), 'thickness'), (dict(trail=-1), 'trail'), (dict(trail=16), 'trail'), (dict(alpha=0.0), 'alpha'),
                     (dict(alpha=1.01), 'alpha'), (dict(pad=65), 'pad'), (dict(pad=-1), 'pad'), (dict(label_scale=0), 'label_scale'),
                     (dict(label_scale=9), 'label_scale'), (dict(labels=[1, 2, 3]), 'labels'), (dict(labels=[0.5, 1.0]), 'labels'),
                     (dict(status=[[0, 1]]), 'status'), (dict(landmarks=np.zeros((2, 9, 2), F32)), 'landmarks'),
                     (dict(grow=float('nan')), 'grow')):
        with pytest.raises(ValueError, match=word):
            A.plan_annotate(photos, boxes, 10, **kw)
    with pytest.raises(ValueError, match='65535'):
        A.plan_annotate(photos, [(0, 0, 0, 2, 2)] * 65536, 10)
    with pytest.raises(ValueError, match='exactly one'):
        A.plan_annotate_clip(photos, None, None, 10)
    with pytest.raises(ValueError, match='exactly one'):
        A.plan_annotate_clip(photos, boxes, object(), 10)


def test_the_script_refuses_annotate_without_out_dir_and_with_redact(tmp_path):
    script = os.path.join(ROOT, 'scripts', 'detect.py')
    common = ['--configs', 'none.yaml', '--checkpoint', 'none.pt', '--images-dir', str(tmp_path)]
    with pytest.raises(ValueError, match='--out-dir'):
        D._run_script(script, common + ['--annotate'])
    with pytest.raises(ValueError, match='--redact'):
        D._run_script(script, common + ['--annotate', '--redact', 'pixelate', '--out-dir', str(tmp_path / 'o')])
    for extra in (['--draw', 'points'], ['--trail', '2'], ['--marker-size', '3']):
        with pytest.raises(ValueError, match='go with --annotate'):
            D._run_script(script, common + extra)


# ----------------------------------------------------------------------------------------------------------------------------
# the restatement's own properties, on host arrays
# ----------------------------------------------------------------------------------------------------------------------------
def one_mark(photo, row, at, k=1, size=2.5, alpha=1.0, **kw):
    """One row with one marker of style k at `at` over `photo`: the drawn photo and the drawn mask."""
    marks = np.array(at, F32).reshape(1, 1, 1, 2)
    out, _cov, drawn = AN.annotate([photo], [row], AN.POINTS, 1, 8, 1, marks=marks, gstyle=AN.group_styles(size, 1, alpha),
                                   mstyle=AN.mark_styles(k + 1)[k:k + 1], **kw)
    return out[0], drawn[0]


def test_points_are_the_f64_formula_and_keep_what_is_not_finite():
    rows = np.array([(0, 10, 20, 110, 70), (0, 5, 5, 5, 9), (1, 30, 10, 20, 5)], np.int32)
    mu = np.array([[(-1, -1), (1, 1), (0, 0.5)], [(0, 0), (np.nan, 0.25), (np.inf, -np.inf)], [(0.5, 0.5), (-1, 1), (0, 0)]], F32)
    p = AN.points(mu, rows)
    assert p.dtype == F32 and p[0].tolist() == [[10, 20], [110, 70], [60, 57.5]]
    assert p[1, 0].tolist() == [5, 7] and np.isnan(p[1, 1, 0]) and p[1, 1, 1] == 7.5 and p[1, 2, 0] == np.inf and p[1, 2, 1] == -np.inf
    assert p[2, 0].tolist() == [22.5, 6.25], 'an inverted box is not special'


def test_a_draw_nothing_returns_the_photos():
    rows = AN.case_rows(len(AN.ROWS))
    out, covered, drawn = AN.annotate(PHOTOS, rows, 0, 1, 8, 1)
    assert all(np.array_equal(o, p) for o, p in zip(out, PHOTOS)) and not any(d.any() for d in drawn) and covered[0].any()


def test_b_the_pixel_under_a_marker_is_its_colour_and_c_far_pixels_keep_their_bytes():
    photo = PHOTOS[1]
    row = (0, 10, 10, 50, 60)
    for k in range(56):
        for size in (2.0, 2.5, 6.0):
            out, drawn = one_mark(photo, row, (30, 35), k, size)
            assert out[30, 35].tolist() == AN.mark_styles(56)[k, :3].tolist(), (k, size)
            r, c = np.nonzero(drawn)
            assert len(r) and np.maximum(np.abs(r - 30), np.abs(c - 35)).max() <= size + 2
            assert np.array_equal(out[~drawn], photo[~drawn])
    out, drawn = one_mark(photo, row, (np.nan, 35))
    assert not drawn.any() and np.array_equal(out, photo), 'a NaN mark draws nothing'
    out, drawn = one_mark(photo, row, (30.4, 35.7), 0, 2.5, 0.5)
    assert drawn.any() and not (out[30, 35] == AN.mark_styles(1)[0, :3]).all(), 'alpha 0.5 blends'


def test_d_the_frame_is_the_integer_ring_in_the_colour_of_the_status():
    photo = PHOTOS[1]
    y0, x0, y1, x1 = 8, 12, 40, 70
    for thickness in (1, 3):
        for status, colour in ((None, 0), (0, 0), (1, 1), (2, 2), (4, 3), (6, 2), (1 << 20, 3), (5, 1)):
            out, _cov, drawn = AN.annotate([photo], [(0, y0, x0, y1, x1)], AN.BOX, thickness, 8, 1, status=None if status is None else [status])
            ring = np.zeros(photo.shape[:2], bool)
            ring[y0:y1, x0:x1] = True
            ring[y0 + thickness:y1 - thickness, x0 + thickness:x1 - thickness] = False
            assert np.array_equal(drawn[0], ring)
            assert (out[0][ring] == AN.PALETTE[colour]).all() and np.array_equal(out[0][~ring], photo[~ring])


def test_e_a_lost_row_draws_its_frame_and_label_only_and_f_a_flagged_hull_draws_nothing():
    photo = PHOTOS[1]
    rows = np.array([(0, 8, 12, 48, 70)], np.int32)
    marks = AN.case_marks(rows, 10, 2, 5)
    poses = np.random.RandomState(1).uniform(-0.8, 0.8, (1, 10, 2)).astype(F32)
    edges, flags = HR.hull_fit(poses, rows, np.full(1, 1.25, F32))
    assert flags[0] == 0
    kw = dict(marks=marks, gstyle=AN.group_styles(2.5, 2), mstyle=AN.mark_styles(10), labels=[42])
    full, _c, _d = AN.annotate([photo], rows, AN.ALL, 2, 5, 1, edges=edges, status=[0], **kw)
    lost, _c, _d = AN.annotate([photo], rows, AN.ALL, 2, 5, 1, edges=edges, status=[1], **kw)
    only, _c, _d = AN.annotate([photo], rows, AN.BOX | AN.LABEL, 2, 5, 1, status=[1], labels=[42])
    assert np.array_equal(lost[0], only[0]) and not np.array_equal(full[0], lost[0])
    hull, _c, drawn = AN.annotate([photo], rows, AN.HULL, 2, 5, 1, edges=edges)
    assert drawn[0].any() and not drawn[0][28, 40], 'an outline, not a filled hull'
    bad = poses.copy()
    bad[0, 3, 1] = np.nan
    e2, f2 = HR.hull_fit(bad, rows, np.full(1, 1.25, F32))
    assert f2[0] & 1
    out, _c, drawn = AN.annotate([photo], rows, AN.HULL, 2, 5, 1, edges=e2)
    assert not drawn[0].any() and np.array_equal(out[0], photo)


def test_g_marks_on_a_pixel_centre_are_symmetric_and_up_is_down_flipped():
    flat = np.full((41, 41, 3), 90, np.uint8)
    row = (0, 2, 2, 39, 39)
    patch = {}
    for k in range(0, 56, 8):
        for size in (1.0, 2.5, 6.0):
            patch[AN.SHAPES[k // 8], size] = one_mark(flat, row, (20, 20), k, size)[0][8:33, 8:33, 0].astype(int) - 90
    for (shape, size), p in patch.items():
        assert p.any()
        if shape in 'osd+x':
            assert np.array_equal(p, p[::-1]) and np.array_equal(p, p[:, ::-1]), (shape, size)
            assert np.array_equal(p, p.T), (shape, size)
        else:
            assert np.array_equal(p, p[:, ::-1]) and not np.array_equal(p, p[::-1]), (shape, size)
    # '^' is 'v' flipped: in the blend's weights, which the colours of the two styles share but for their hue; compare the drawn masks
    for size in (1.0, 2.5, 6.0):
        v, up = one_mark(flat, row, (20, 20), 0, size)[1], one_mark(flat, row, (20, 20), 32, size)[1]
        assert np.array_equal(v, up[::-1]) and v.any()
    same = AN.mark_styles(40)
    same[32, :3] = same[0, :3]
    a = AN.annotate([flat], [row], AN.POINTS, 1, 8, 1, marks=np.array([20, 20], F32).reshape(1, 1, 1, 2), gstyle=AN.group_styles(2.5, 1),
                    mstyle=same[0:1])[0][0]
    b = AN.annotate([flat], [row], AN.POINTS, 1, 8, 1, marks=np.array([20, 20], F32).reshape(1, 1, 1, 2), gstyle=AN.group_styles(2.5, 1),
                    mstyle=same[32:33])[0][0]
    assert np.array_equal(a, b[::-1])


def test_the_label_is_the_font_in_white_on_the_rows_colour():
    flat = np.full((40, 60, 3), 7, np.uint8)
    for scale in (1, 2):
        out, _c, drawn = AN.annotate([flat], [(0, 3, 4, 38, 58)], AN.LABEL, 2, 0, scale, labels=[907], status=[4])
        oy, ox = 3 + 2, 4 + 2
        assert drawn[0].sum() == 9 * scale * 19 * scale and drawn[0][oy:oy + 9 * scale, ox:ox + 19 * scale].all()
        white = (out[0] == 255).all(axis=2)
        for i, d in enumerate((9, 0, 7)):
            glyph = white[oy + scale:oy + 8 * scale:scale, ox + scale * (1 + 6 * i):ox + scale * (6 + 6 * i):scale]
            assert np.array_equal(glyph, AN.FONT_BITS[d]), (scale, d)
        assert (out[0][drawn[0] & ~white] == AN.PALETTE[3]).all()
    for bad in (-1, 10000):
        out, _c, drawn = AN.annotate([flat], [(0, 3, 4, 38, 58)], AN.LABEL, 2, 0, 1, labels=[bad])
        assert not drawn[0].any()
    out, _c, drawn = AN.annotate([flat], [(0, 3, 4, 12, 14)], AN.LABEL, 1, 4, 2, labels=[1234])
    assert drawn[0].any() and not drawn[0][:3].any() and not drawn[0][12:].any() and not drawn[0][:, 14:].any(), 'clipped to the box'


def test_h_rows_one_by_one_give_the_bytes_of_one_pass_and_i_the_later_row_lies_over_the_earlier():
    rows = np.array([(1, 5, 5, 30, 30), (1, 34, 40, 60, 75), (0, 2, 2, 20, 20)], np.int32)
    marks = AN.case_marks(rows, 10, 1, 4)
    kw = dict(gstyle=AN.group_styles(2.5, 1), mstyle=AN.mark_styles(10))
    whole, _c, _d = AN.annotate(PHOTOS, rows, AN.POINTS | AN.BOX, 1, 4, 1, marks=marks, **kw)
    parts = PHOTOS
    for b in range(3):
        parts, _c, _d = AN.annotate(parts, rows[b:b + 1], AN.POINTS | AN.BOX, 1, 4, 1, marks=marks[:, b:b + 1], **kw)
    assert all(np.array_equal(a, b) for a, b in zip(whole, parts))
    two = np.array([(1, 10, 10, 40, 40), (1, 20, 20, 50, 50)], np.int32)
    out, _c, _d = AN.annotate(PHOTOS, two, AN.BOX, 2, 0, 1, status=[0, 1])
    assert (out[1][20, 25] == AN.PALETTE[1]).all() and (out[1][39, 25] == AN.PALETTE[0]).all() and (out[1][20, 39] == AN.PALETTE[1]).all()
    out, _c, _d = AN.annotate(PHOTOS, two[::-1], AN.BOX, 2, 0, 1, status=[1, 0])
    assert (out[1][20, 39] == AN.PALETTE[0]).all()
