"""The landmark-hull mask of morph, host side (no GPU): the ABI of imm_hull_fit / imm_morph_hull_u8 and their argument validation, the
wrapper and plan_morph refusals, the hull rule of the restatement (tests/hull_reference.py) against exact rational arithmetic,
hand-derived known answers, and the f32 restatement of the morph with the mask against the f64 one on the GPU test's case."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colour_reference as CO                                               # noqa: E402
import hull_reference as HR                                                 # noqa: E402
import morph_reference as R                                                 # noqa: E402
import unalign_reference as UR                                              # noqa: E402
import warp_reference as WR                                                 # noqa: E402

from imm_amd import morphing as MP                                          # noqa: E402  (imports without a GPU)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAMES = ['imm_hull_fit', 'imm_morph_hull_u8']


# ----------------------------------------------------------------------------------------------------------------------------
# ABI and validation
# ----------------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_hull_entry_points():
    from imm_amd import _lib as L
    assert L.ABI_VERSION >= 33
    header = open(os.path.join(ROOT, 'include', 'imm_hull.h')).read()
    assert L.symbols('imm_hull.h') == NAMES
    for text in ('THE RULE', 'Hull fit (imm_hull_fit)', 'Weight.', 'Morph with the mask (imm_morph_hull_u8)', 'rounded separately',
                 'in index order', 'CANDIDATE', 'ties go to the lowest j', 'No compaction', '(0, 0, +inf)', '(0, 0, -inf)', 'bit 0', 'bit 1',
                 'Ownership does not', 'Consequences'):
        assert text in header, text
    src = open(os.path.join(ROOT, 'imm_amd', 'csrc', 'hull.hip')).read()
    assert 'fp contract(off)' in src and '__host__ __device__' in src and 'atomic' not in src.lower() and 'asm' not in src.lower()
    morph = open(os.path.join(ROOT, 'imm_amd', 'csrc', 'morph.hip')).read()
    assert 'imm_morph_hull_u8' in morph and 'bool HULL = false' in morph
    assert 'morph_u8_kernel<true>' in morph and 'morph_u8_kernel<false>' in morph, 'the two earlier launches keep their spelling'


def test_hull_entry_points_validate_their_arguments_without_a_device():
    from imm_amd import _lib as L
    lib = L.load()
    one, two, three = C.c_void_p(16), C.c_void_p(32), C.c_void_p(48)     # non-null pointers that are never read: validation comes first
    #       poses boxes grow K  n  edges flags stream
    good = [one, one, one, 10, 3, two, three, None]
    bad_args = [(i, None) for i in (0, 1, 2, 5, 6)] + [(3, 0), (3, -1), (3, 81), (4, 0), (4, -1), (4, 65536)]
    for i, bad in bad_args:
        args = list(good)
        args[i] = bad
        assert lib.imm_hull_fit(*args) == -1, (i, bad)
        assert b'hull_fit' in lib.imm_last_error()
    #       src  dst  offs hw  n_img donor doffs dhw n_donor boxes dboxes links ramp texture ctrl coef_a coef_b gain edges soft K   M   n  pixels stream
    good = [one, two, one, one, 2, three, one, one, 3, one, one, one, one, one, one, one, one, one, one, one, 10, 18, 3, 100, None]
    bad_args = [(i, None) for i in (0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 18, 19)]
    bad_args += [(1, one), (5, two), (4, 0), (8, 0), (8, -1), (20, 0), (20, -1), (20, 81), (21, 2), (21, 81), (22, 0), (22, 65536), (23, 0),
                 (23, -5)]
    for gain in (one, None):                                             # gain is nullable: NULL selects the instantiation without colour
        for i, bad in bad_args:
            args = list(good)
            args[17] = gain
            args[i] = bad
            assert lib.imm_morph_hull_u8(*args) == -1, (i, bad)
            assert b'morph_hull_u8' in lib.imm_last_error()


def test_wrapper_refusals_come_before_any_device_call():
    from imm_amd import ops
    z = lambda *sh, **kw: torch.zeros(*sh, **kw)           # host tensors: a wrapper that got as far as the library would fault
    n, K, M = 2, 10, 18
    poses, boxes, grow, edges, flags = z(n, K, 2), z(n, 5, dtype=torch.int32), z(n), z(n, K, 3), z(n, dtype=torch.int32)
    for kw, match in ((dict(poses=z(n, K)), 'poses'), (dict(poses=z(n, K, 3)), 'poses'), (dict(poses=poses.double()), 'poses'),
                      (dict(poses=z(2 * n, K, 2)[::2]), 'poses'), (dict(poses=z(n, 81, 2)), 'landmarks'), (dict(poses=poses[:0]), 'rows'),
                      (dict(boxes=boxes.long()), 'boxes'), (dict(boxes=z(n, 4, dtype=torch.int32)), 'boxes'), (dict(grow=z(n, 1)), 'grow'),
                      (dict(grow=grow.double()), 'grow'), (dict(edges=z(n, K, 2)), 'edges'), (dict(edges=z(n + 1, K, 3)), 'edges'),
                      (dict(flags=flags.long()), 'flags'), (dict(flags=flags[:1]), 'flags')):
        args = dict(poses=poses, boxes=boxes, grow=grow, edges=edges, flags=flags)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.hull_fit(**args)
    src, dst, don = z(64, dtype=torch.uint8), z(64, dtype=torch.uint8), z(48, dtype=torch.uint8)
    offs, hw, doffs, dhw = z(1, dtype=torch.int64), z(1, 2, dtype=torch.int32), z(2, dtype=torch.int64), z(2, 2, dtype=torch.int32)
    links, ramp, tex, ctrl, coef, gain, soft = z(n, 2, dtype=torch.int32), z(n, 2), z(n), z(n, M, 2), z(n, M + 3, 2), z(n, 3, 2), z(n)
    for kw, match in ((dict(edges=z(n, K)), 'edges'), (dict(edges=z(n, K, 2)), 'edges'), (dict(edges=z(n + 1, K, 3)), 'edges'),
                      (dict(edges=z(n, 81, 3)), 'edges'), (dict(edges=edges.double()), 'edges'), (dict(inv_soft=z(n, 1)), 'inv_soft'),
                      (dict(inv_soft=soft.double()), 'inv_soft'), (dict(gain=z(n, 3)), 'gain'), (dict(gain=gain.double()), 'gain'),
                      (dict(dst=src), 'copy of src'), (dict(donor=dst), 'never dst'), (dict(texture=z(n, 1)), 'texture'),
                      (dict(ctrl=z(n, 2, 2)), 'morph_hull_u8 serves'), (dict(max_box_pixels=0), 'max_box_pixels')):
        for g in (gain, None):
            args = dict(src=src, dst=dst, offsets=offs, hw=hw, donor=don, donor_offsets=doffs, donor_hw=dhw, boxes=boxes, donor_boxes=boxes,
                        links=links, inv_ramp=ramp, texture=tex, ctrl=ctrl, coef_a=coef, coef_b=coef, gain=g, edges=edges, inv_soft=soft,
                        max_box_pixels=9)
            args.update(kw)
            if 'gain' in kw and g is None:
                continue
            with pytest.raises(ValueError, match=match):
                ops.morph_hull_u8(**args)


# ----------------------------------------------------------------------------------------------------------------------------
# plan_morph, PhotoMorph and the script's arguments
# ----------------------------------------------------------------------------------------------------------------------------
def test_plan_morph_checks_the_mask():
    photos = [np.zeros((40, 50, 3), np.uint8), np.zeros((30, 30, 3), np.uint8)]
    donors = [np.zeros((20, 25, 3), np.uint8), np.zeros((35, 30), np.uint8)]
    good = dict(photos=photos, donors=donors, boxes=None, donor_boxes=None, shape=0.5, texture=None, feather=0.125, K=10)
    plan = MP.plan_morph(**good)
    assert len(vars(plan)) == 21 and plan.mask is None and plan.grow.tolist() == [1.25, 1.25] and plan.grow.dtype == F32
    assert np.array_equal(plan.mask_feather, np.full(2, 0.1, F32))
    # mask=None: the fifteen values of a call without the keyword, whatever grow and mask_feather are
    for kw in (dict(mask=None), dict(mask=None, grow=3.0, mask_feather=0.5), dict(mask='hull'), dict(colour=0.0, mask=None)):
        other = MP.plan_morph(**dict(good, **kw))
        assert len(vars(other)) == 21 and other.mask == kw.get('mask')
        for x, y in ((getattr(plan, k), getattr(other, k)) for k in MP.MorphPlan.FIELDS[:15]):
            if isinstance(x, list):                                          # the decoded photos
                assert len(x) == len(y) and all(np.array_equal(a, b) for a, b in zip(x, y))
            else:
                assert (x is None and y is None) or (type(x) is type(y) and np.array_equal(x, y))
    plan = MP.plan_morph(mask='hull', grow=[0.5, 16.0], mask_feather=[0.0, 1.0], **good)
    assert plan.mask == 'hull' and plan.grow.tolist() == [0.5, 16.0] and plan.mask_feather.tolist() == [0.0, 1.0]
    # inv_soft = f32(1 / max(1, mask_feather * min(H, W))): the whole-photo boxes are 40 x 50 and 30 x 30
    assert plan.inv_soft.dtype == F32 and plan.inv_soft.tolist() == [1.0, F32(1.0 / 30.0)]
    assert MP.plan_morph(mask='hull', mask_feather=0.25, **good).inv_soft.tolist() == [F32(0.1), F32(1.0 / 7.5)]
    assert np.array_equal(MP.hull_inv_soft([(0, 0, 0, 3, 100)], [0.1]), [F32(1.0)]), 'at least one pixel'
    assert np.array_equal(plan.inv_soft, HR.inv_soft(plan.rows, [0.0, 1.0]))
    for kw, match in ((dict(mask='ellipse'), 'mask'), (dict(mask='Hull'), 'mask'), (dict(mask=1), 'mask'), (dict(mask=True), 'mask'),
                      (dict(grow=0.0), 'grow'), (dict(grow=-1.0), 'grow'), (dict(grow=16.5), 'grow'), (dict(grow=float('nan')), 'grow'),
                      (dict(grow=float('inf')), 'grow'), (dict(grow=[1.0, 2.0, 3.0]), 'grow'), (dict(grow=[[1.0, 2.0]]), 'grow'),
                      (dict(mask_feather=-0.01), 'mask_feather'), (dict(mask_feather=1.01), 'mask_feather'),
                      (dict(mask_feather=float('nan')), 'mask_feather'), (dict(mask_feather=[0.1] * 3), 'mask_feather')):
        for mask in ('hull', None):                                          # refused whether or not the mask is asked for
            args = dict(good, mask=mask)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                MP.plan_morph(**args)
    # PhotoMorph: the fields, their defaults for a caller of the earlier signature, and hull_weight on host arrays
    pm = MP.PhotoMorph(None, None, None, np.zeros((2, 5)), np.zeros((2, 5)), None, None, None, None, [0, 1], [1, 0], 0.0, 2, [0.5, 1.0], 2.0,
                       'gain', 'flags')
    assert pm.mask is None and pm.hull_edges is None and pm.hull_flags is None and pm.grow is None and pm.inv_soft is None
    with pytest.raises(ValueError, match='hull'):
        pm.hull_weight(0)
    poses, rows, grow = HR.case_inputs(HR.SQUARE, (16, 16), 1.0)
    edges, flags = HR.hull_fit(poses, rows, grow)
    pm = MP.PhotoMorph(None, None, None, rows, rows, None, None, None, None, [0], [1], 0.0, 2, mask='hull', grow=grow, mask_feather=[0.25],
                       inv_soft=[0.25], hull_edges=edges, hull_flags=flags)
    w = pm.hull_weight(0)
    assert w.dtype == F32 and w.shape == (16, 16) and np.array_equal(w, HR.weight_f32(edges[0], 0.25, 16, 16))
    # by hand: 0 up to the square's edge at 4 and 12, then a quarter more per pixel, 1 from four pixels inside
    assert w[8].tolist() == [0, 0, 0, 0, 0, 0.25, 0.5, 0.75, 1, 0.75, 0.5, 0.25, 0, 0, 0, 0] and np.array_equal(w, w.T) and w[4].max() == 0


def test_generate_script_parses_the_mask_arguments(capsys):
    spec = importlib.util.spec_from_file_location('generate_script', os.path.join(ROOT, 'scripts', 'generate.py'))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    need = ['--configs', 'c.yaml', '--checkpoint', 'm.pt', '--appearance-dir', 'photos']
    args = script.build_parser().parse_args(need + ['--morph'])
    assert args.mask is None and args.grow is None and args.mask_feather is None
    args = script.build_parser().parse_args(need + ['--morph', '--mask', 'hull'])
    assert args.mask == 'hull' and args.grow is None and args.mask_feather is None
    args = script.build_parser().parse_args(need + ['--morph', '--mask', 'hull', '--grow', '1.5', '--mask-feather', '0.2'])
    assert (args.mask, args.grow, args.mask_feather) == ('hull', 1.5, 0.2)
    for bad in (['--mask', 'ellipse'], ['--mask'], ['--grow', 'big'], ['--mask-feather']):
        with pytest.raises(SystemExit):
            script.build_parser().parse_args(need + ['--morph'] + bad)
    capsys.readouterr()
    assert '--mask hull' in script.__doc__ and '--grow' in script.__doc__ and '--mask-feather' in script.__doc__


# ----------------------------------------------------------------------------------------------------------------------------
# the hull rule against exact arithmetic
# ----------------------------------------------------------------------------------------------------------------------------
def _check_against_exact(poses, rows, grow, what):
    edges, flags = HR.hull_fit(poses, rows, grow)
    assert edges.dtype == F32 and flags.dtype == np.int32
    for b in range(len(rows)):
        if flags[b] & 1:
            assert np.array_equal(edges[b], np.tile(HR.NO_HULL, (poses.shape[1], 1))), (what, b)
            continue
        has, inner = HR.hull_exact(poses[b], rows[b], grow[b])
        assert bool(flags[b] & 2) == (int(has.sum()) < 3 or not inner), (what, b)
        if flags[b]:
            assert np.array_equal(edges[b], np.tile(HR.NO_HULL, (poses.shape[1], 1))), (what, b)
            continue
        got = ~np.isposinf(edges[b, :, 2])
        assert np.array_equal(got, has), (what, b, got, has)
        assert np.array_equal(edges[b][~got], np.tile(HR.NO_WINNER, (int((~got).sum()), 1)))
        live = edges[b][got].astype(np.float64)
        assert np.allclose(np.hypot(live[:, 0], live[:, 1]), 1.0, rtol=0, atol=1e-6), 'unit normals'
    return edges, flags


@pytest.mark.parametrize('name,points,hw,want', HR.CASES, ids=[c[0] for c in HR.CASES])
def test_hull_rule_against_exact_arithmetic(name, points, hw, want):
    """The restatement's slots that have a winner against exact rational arithmetic on the same f32 inputs (these inputs are small
    dyadic numbers, so float64 is exact on them as well, collinear points stay collinear and the two must agree slot by slot)."""
    for grow in (1.0, 1.25, 0.5):
        poses, rows, g = HR.case_inputs(points, hw, grow)
        edges, flags = _check_against_exact(poses, rows, g, name)
        assert flags.tolist() == [want], (name, grow)
        # the box corner never enters
        e2, f2 = HR.hull_fit(*HR.case_inputs(points, hw, grow, corner=(-100, 70000)))
        assert np.array_equal(e2.view(np.uint32), edges.view(np.uint32)) and np.array_equal(f2, flags)
    poses, rows, g = HR.case_inputs(points, hw, 1.0)
    edges, flags = HR.hull_fit(poses, rows, g)
    w = HR.weight_f32(edges[0], 1e30, *hw)
    if want:
        assert not w.any(), 'a flagged row has the weight 0 everywhere'
    elif np.array_equal((poses[0].astype(np.float64) + 1) * (0.5 * np.array(hw)), np.array(points)):       # sides that are powers of two
        # a hard edge: the weight is 1 exactly at the lattice points strictly inside the polygon (integer vertices, exact in f32)
        hull = [points[i] for i in _ring(points)]
        assert np.array_equal(w > 0, HR.inside_count(hull, *hw)) and set(np.unique(w).tolist()) <= {0.0, 1.0} and w.any()


def _ring(points):
    """The indices of the hull's vertices in order (gift wrapping in integers; the hand-made cases only)."""
    pts = [tuple(p) for p in points]
    start = min(range(len(pts)), key=lambda i: pts[i])
    ring, i = [start], start
    while True:
        best = None
        for j in range(len(pts)):
            if pts[j] == pts[i]:
                continue
            ey, ex = pts[j][0] - pts[i][0], pts[j][1] - pts[i][1]
            if all(ey * (q[1] - pts[i][1]) - ex * (q[0] - pts[i][0]) >= 0 for q in pts):
                if best is None or ey * ey + ex * ex > (pts[best][0] - pts[i][0]) ** 2 + (pts[best][1] - pts[i][1]) ** 2:
                    best = j
        if best is None or pts[best] == pts[start]:
            return ring
        ring.append(best)
        i = best


@pytest.mark.parametrize('K,m', R.KERNEL_SHAPES)
def test_hull_rule_on_the_kernel_case(K, m):
    """morph's kernel case, the blended poses of its 15 rows: the slots with a winner are those of exact arithmetic, 3 per row at K = 3,
    4 to 8 at K = 10 and 9 to 14 at K = 64; the NaN row has flag bit 0 and no hull."""
    case, poses = HR.kernel_poses(K, m)
    rows = case[1]
    for grow in (1.25, 1.0):
        edges, flags = _check_against_exact(poses, rows, np.full(len(rows), grow, F32), K)
        assert flags.tolist() == [3 * int(b == R.NAN_ROW) for b in range(len(rows))], "a NaN pose: bit 0, and no line has every point inside: bit 1"
        counts = [int((~np.isposinf(edges[b, :, 2])).sum()) for b in range(len(rows)) if b != R.NAN_ROW]
        lo, hi = {3: (3, 3), 10: (4, 8), 64: (9, 14)}[K]
        print('\nHULL K=%d grow=%g: vertices per row %s' % (K, grow, counts))
        assert min(counts) >= lo and max(counts) <= hi, counts


def test_unit_square_known_answer():
    """The square of side 1 about the centre of the frame (poses +-0.5) in a 16 x 16 box at grow = 1: corners (4, 4), (4, 12), (12, 12),
    (12, 4) as (y, x).  By hand, slot 0, corner (4, 4): only (12, 4) has every corner on its inner side (e = (8, 0), the expression is
    8 (x_k - 4) >= 0), so len = 8, ny = -0 / 8, nx = 8 / 8 = 1, d = -(1 * 4) = -4: the line c - 4.  Likewise corner (4, 12) -> (4, 4):
    r - 4; corner (12, 12) -> (4, 12): 12 - c; corner (12, 4) -> (12, 12): 12 - r."""
    poses = np.array([[(-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5)]], F32)
    rows = np.array([(0, 7, 9, 23, 25)], np.int32)
    edges, flags = HR.hull_fit(poses, rows, np.ones(1, F32))
    assert flags.tolist() == [0]
    assert edges[0].tolist() == [[0.0, 1.0, -4.0], [1.0, 0.0, -4.0], [0.0, -1.0, 12.0], [-1.0, 0.0, 12.0]]
    # grown by 1.25 about the centre (8, 8): corners at 3 and 13
    edges, flags = HR.hull_fit(poses, rows, np.full(1, 1.25, F32))
    assert edges[0].tolist() == [[0.0, 1.0, -3.0], [1.0, 0.0, -3.0], [0.0, -1.0, 13.0], [-1.0, 0.0, 13.0]] and flags.tolist() == [0]
    w = HR.weight_f32(edges[0], 0.5, 16, 16)
    assert w[8].tolist() == [0, 0, 0, 0, 0.5, 1, 1, 1, 1, 1, 1, 1, 0.5, 0, 0, 0]
    assert np.array_equal(w, HR.weight_f64(edges[0], 0.5, 16, 16).astype(F32))


# vertices at half pixels, so that no pixel lies on the polygon's edge (checked below in integers): (y, x) in a 32 x 32 box
FLAT_POLYGON = [(15.5, 3.5), (27.5, 12.5), (19.5, 27.5), (3.5, 24.5)]


def flat_case():
    """Two flat photos and one row whose FOUR landmarks are FLAT_POLYGON on both sides (the spline is the identity, coefficients exactly
    zero): (photo, donor, rows, drows, poses f32 [1, 4, 2], the bool [32, 32] of the pixels strictly inside the polygon)."""
    photo, donor = CO.flat_photo(48, 57, (200, 17, 99)), CO.flat_photo(30, 21, (90, 30, 140))
    rows, drows = np.array([(0, 4, 20, 36, 52)], dtype=np.int32), np.array([(0, 3, 2, 25, 18)], dtype=np.int32)
    poses = HR.poses_of(FLAT_POLYGON, 32, 32)[None]
    assert np.array_equal((poses.astype(np.float64) + 1) * 16, np.array([FLAT_POLYGON])), 'exact in f32'
    twice = [(int(2 * y), int(2 * x)) for y, x in FLAT_POLYGON]
    r, c = 2 * np.arange(32, dtype=np.int64)[:, None], 2 * np.arange(32, dtype=np.int64)[None, :]
    cross = [(by - ay) * (c - ax) - (bx - ax) * (r - ay) for (ay, ax), (by, bx) in zip(twice, twice[1:] + twice[:1])]
    assert all((x != 0).all() for x in cross), 'no pixel on an edge'
    inside = np.all([x > 0 for x in cross], axis=0) | np.all([x < 0 for x in cross], axis=0)
    return photo, donor, rows, drows, poses, inside


def test_flat_photos_hard_edge_known_answer():
    """Two flat photos of colours A and B, shape = 0, texture = 1, feather = 0 and a hard edge (inv_soft = 1e30): the output is B exactly
    at the pixels strictly inside the polygon and A elsewhere, and their number is the count of lattice points inside it."""
    photo, donor, rows, drows, poses, inside = flat_case()
    edges, flags = HR.hull_fit(poses, rows, np.ones(1, F32))
    assert flags.tolist() == [0] and 300 < inside.sum() < 400
    coef_a, coef_b, ctrl, fflags, _cond = R.fit2_f64(poses, poses, R.blend_f32(poses, poses, [0.0]), 2, 0.0)
    assert not fflags.any() and not coef_a.any() and not coef_b.any()
    ramp = WR.inv_ramp(rows, 0.0)
    want = photo.copy()
    want[4:36, 20:52][inside] = (90, 30, 140)
    for fn in (HR.morph_f64, HR.morph_f32):
        out, cov = fn([photo], rows, [donor], drows, ctrl, coef_a, coef_b, [1.0], ramp, edges, np.array([1e30], F32))
        assert np.array_equal(out[0], want) and cov[0].sum() == inside.sum() and np.array_equal(cov[0][4:36, 20:52], inside)
        # and with a gain that turns B into C
        gain = np.tile(np.array([1.0, 7.0], F32), (1, 3, 1))
        out, _c = fn([photo], rows, [donor], drows, ctrl, coef_a, coef_b, [1.0], ramp, edges, np.array([1e30], F32), gain)
        assert (out[0][4:36, 20:52][inside] == (97, 37, 147)).all() and np.array_equal(out[0][~cov[0]], photo[~cov[0]])


# ----------------------------------------------------------------------------------------------------------------------------
# the cap, on the restatements alone
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,m', R.KERNEL_SHAPES)
def test_f32_restatement_against_f64(K, m):
    """morph's kernel case at grow = 1.25 and mask_feather 0.1 and 0.25, for every lam and feather, with and without colour_reference's
    gains: morph_f32 against morph_f64, both driven by the f32-rounded coefficients and the restatement's f32 lines, stays within
    unalign_reference.within_cap (one grey level, 0.5 % of the pixels with w > 0), and the two agree on which pixels have w > 0.
    Found: 0 of 315 (K = 3) and 0 to 1 of 883 (K = 10) and of 1 502 (K = 64) such pixels differ, by one grey level."""
    case, poses = HR.kernel_poses(K, m)
    photos, rows, donors, drows, mu_a, mu_b, shape, texture = case
    n = len(rows)
    edges, hflags = HR.hull_fit(poses, rows, np.full(n, HR.GROW, F32))
    assert hflags.tolist() == [3 * int(b == R.NAN_ROW) for b in range(n)]
    gain, _gflags, _amount = CO.morph_gains(case)
    for lam in R.LAMS:
        _case, _poses, coef_a, coef_b, ctrl, flags, cond = R.fitted_case(K, m, lam)
        ca, cb = coef_a.astype(F32), coef_b.astype(F32)
        for feather in R.FEATHERS:
            ramp = WR.inv_ramp(rows, feather)
            plain32, box = R.morph_f32(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp)
            for mf in HR.MASK_FEATHERS:
                soft = HR.inv_soft(rows, mf)
                for g in (None, gain):
                    ref64, covered = HR.morph_f64(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp, edges, soft, g)
                    ref32, cov32 = HR.morph_f32(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp, edges, soft, g)
                    n_diff, worst, _near, n_cov = UR.within_cap(ref32, ref64, covered, WR.no_band(photos))
                    print('\nHULL MORPH f32 vs f64 K=%d anchors=%d lam=%g feather=%g mask_feather=%g gain=%s: %d of %d pixels with w > 0 '
                          'differ (max %d)' % (K, m, lam, feather, mf, g is not None, n_diff, n_cov, worst))
                    assert all(np.array_equal(x, y) for x, y in zip(covered, cov32)), 'the two disagree on which pixels have w > 0'
                    assert n_cov > 300 and all(not (c & ~bx).any() for c, bx in zip(covered, box)), 'the mask only takes pixels away'
                    assert sum(int(c.sum()) for c in covered) < 0.9 * sum(int(bx.sum()) for bx in box)
                    assert all(np.array_equal(a[~c], p[~c]) for a, p, c in zip(ref32, photos, covered))
    # a hull that holds the whole box at w = 1 is the morph without the mask, in both restatements, with and without a gain
    whole = np.tile(np.array([[0.0, 0.0, 1.0]], F32), (n, K, 1))
    one = np.ones(n, F32)
    for g, plain in ((None, R.morph_f32(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp)[0]),
                     (gain, CO.morph_f32(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp, gain)[0])):
        same, _c = HR.morph_f32(photos, rows, donors, drows, ctrl, ca, cb, texture, ramp, whole, one, g)
        assert all(np.array_equal(a, b) for a, b in zip(same, plain))
