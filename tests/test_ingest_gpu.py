"""The four kernels every photo passes through first, on a real MI355X, on guarded buffers (tests/guarded.py): imm_tps_warp and
imm_tps_warp_pad, imm_resize_crop_u8 (plain and box mode), imm_align_coeffs and imm_align_warp_u8, and the keypoint epilogue of the
pose head.

Every kernel output comes from guarded.out() (NaN body between 0xFF bands) and every operand from guarded.inp(): a store one pixel,
one row or one sample past a tensor lands in a band (check_guards after every test), a load past an operand that reaches arithmetic
turns the result NaN, and an element the kernel leaves unwritten stays NaN.  Where the arithmetic can be made exact it is
(tests/ingest_data.py, validated without a GPU by tests/test_ingest_cpu.py) and the comparison is bit for bit: integer shifts and
flips through the thin-plate-spline warp and through the align warp in both source modes, integer matrix products through
imm_align_coeffs, and the resize against its f32 restatement, from photo buffers packed with no padding at odd byte offsets whose last
photo ends on the last byte before the guard band.  The remaining comparisons keep the bounds of the files they extend.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alignment_reference as R                                             # noqa: E402
import guarded                                                              # noqa: E402
import ingest_data as D                                                     # noqa: E402
from guarded import untouched                                               # noqa: E402
from oracle import image_oracle as IO                                       # noqa: E402
from oracle import tps_oracle as T                                          # noqa: E402
from test_alignment_gpu import BOXES as ALIGN_BOXES, PHOTOS as ALIGN_BOX_PHOTOS, warp_bound   # noqa: E402
from test_keypoints_gpu import KP_BOUND, crop_to_box, restate               # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = torch.float32
S = D.S


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


@pytest.fixture(autouse=True)
def _guards_intact():
    """After every test: no kernel wrote outside a tensor it was handed."""
    guarded.reset()
    yield
    guarded.check_guards()


def inp(a):
    return guarded.inp(torch.from_numpy(np.ascontiguousarray(a)), DEV, depth=2)


def done():
    torch.cuda.synchronize()
    guarded.check_guards()


def close_abs(got, ref, atol, what):
    """guarded.close with an absolute bound: every element within atol, a NaN or an inf fails."""
    ref = torch.as_tensor(np.asarray(ref, np.float64))
    guarded.close(torch.as_tensor(got), ref, 0.0, atol / (float(ref.abs().max()) + 1e-30), what)


# ----------------------------------------------------------------------------------------------------------------------------
# A. imm_tps_warp, exact
# ----------------------------------------------------------------------------------------------------------------------------
def run_tps(ops, img, w, basis_t, ld_src, ld_dst, ld_rest, off=0):
    """imm_tps_warp of img [B, H, W, C] read as channels [off, off + C) of an ld_src-wide buffer (the other channels NaN) into
    channels [off, off + C) of an ld_dst-wide dst, dst_c0 and (C > 1) the first C - 1 channels of an ld_rest-wide dst_rest.  Returns
    the three as host arrays after the guard check; the channels around them must be untouched."""
    B, H, W, C = img.shape
    wide = np.full((B, H, W, ld_src), np.nan, np.float32)
    wide[..., off:off + C] = img
    src = inp(wide)[..., off:off + C]
    dst_buf = guarded.out((B, H, W, ld_dst), F32, DEV)
    c0 = guarded.out((B, H, W), F32, DEV)
    rest_buf = guarded.out((B, H, W, ld_rest), F32, DEV) if C > 1 else None
    ops.tps_warp(src, inp(basis_t), inp(w), dst_buf[..., off:off + C], c0, None if C == 1 else rest_buf[..., :C - 1])
    done()
    assert untouched(dst_buf[..., :off]) and untouched(dst_buf[..., off + C:]), 'dst: channels outside [off, off + c) were written'
    if C > 1:
        assert untouched(rest_buf[..., C - 1:]), 'dst_rest: channels beyond c - 1 were written'
    return (dst_buf[..., off:off + C].cpu().numpy(), c0.cpu().numpy(), None if C == 1 else rest_buf[..., :C - 1].cpu().numpy())


def _tps_layouts():
    out = []
    for shape, sid in zip(D.TPS_EXACT, D.TPS_EXACT_IDS):
        c = shape[3]
        out.append(pytest.param(shape, (c, c, max(c - 1, 1), 0), id=sid + '-dense'))
        out.append(pytest.param(shape, (c + 3, c + 1, c + 2, 0), id=sid + '-wide'))
        if c == 4:
            out.append(pytest.param(shape, (8, 8, 8, 0), id=sid + '-float4_ld8'))       # the float4 path with padding channels
            out.append(pytest.param(shape, (5, 5, 5, 0), id=sid + '-scalar_ld5'))
            # channels 1..4 of an 8-wide buffer: ld % 4 == 0 but every pixel 4 bytes off a 16-byte boundary (the scalar path)
            out.append(pytest.param(shape, (8, 8, 8, 1), id=sid + '-offset_view'))
    return out


@pytest.mark.parametrize('shape,layout', _tps_layouts())
def test_tps_warp_exact(ops, shape, layout):
    """Integer shifts and flips, a different one per sample: the output is the indexed image with exact zeros outside."""
    from imm_amd.data.tps import tps_basis_t
    B, H, W, C, hc, wc = shape
    img, w, expect, inside = D.tps_exact_case(*shape)
    assert 1.0 - inside.mean() >= 0.05 and inside.mean() >= 0.50
    dst, c0, rest = run_tps(ops, img, w, tps_basis_t(H, W, hc, wc), *layout)
    np.testing.assert_array_equal(dst, expect)
    np.testing.assert_array_equal(c0, expect[..., 0])
    if C > 1:
        np.testing.assert_array_equal(rest, expect[..., 1:])


# ----------------------------------------------------------------------------------------------------------------------------
# B. the TPS warps against the oracle at the edges
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,H,W,C,hc,wc', [(13, 19, 23, 2, 3, 3), (5, 31, 47, 5, 4, 5), (9, 24, 40, 8, 3, 3)],
                         ids=['13x19x23x2', '5x31x47x5', '9x24x40x8'])
def test_tps_warp_vs_oracle_guarded(ops, B, H, W, C, hc, wc):
    """Random strong warps as tests/test_tps_gpu.py test_warp_vs_oracle draws them, with its bounds (max 2e-2, mean 2e-4 on 0..255)."""
    from imm_amd.data.tps import tps_basis_t
    rng = np.random.RandomState(B)
    img = (rng.rand(B, H, W, C) * 255).astype(np.float32)
    w = np.stack([T.sample_tps_w(hc, wc, (0.01, 0.05), 20.0, 0.3, 0.4, rng) for _ in range(B)]).astype(np.float32)
    ref = T.warp(img, w, hc, wc)
    assert float((ref == 0).mean()) > 0.01, 'the case should exercise the zero padding'
    dst, c0, rest = run_tps(ops, img, w, tps_basis_t(H, W, hc, wc), C, C, C - 1)
    mean = float(np.mean(np.abs(dst - ref)))
    print('\nTPS WARP %s: max |gpu - oracle| %.3g, mean %.3g' % ((B, H, W, C), float(np.abs(dst - ref).max()), mean))
    close_abs(dst, ref, 2e-2, 'tps_warp dst')
    assert mean < 2e-4
    np.testing.assert_array_equal(c0, dst[..., 0])
    np.testing.assert_array_equal(rest, dst[..., 1:])


@pytest.mark.parametrize('B,H,W,C,hc,wc', [(10, 12, 10, 5, 3, 3), (3, 15, 13, 2, 4, 5)], ids=['10x12x10x5', '3x15x13x2'])
def test_tps_warp_pad_vs_oracle_guarded(ops, B, H, W, C, hc, wc):
    """pad=True with the bounds of tests/test_tps_gpu.py test_padded_warp_vs_oracle (max 2e-2, mean 3e-4); geometry as
    TPSRandomSampler derives it."""
    from imm_amd.data.tps import tps_basis_t
    rng = np.random.RandomState(100 + B)
    img = (rng.rand(B, H, W, C) * 255).astype(np.float32)
    w = np.stack([T.sample_tps_w(hc, wc, (0.01, 0.05), 20.0, 0.3, 0.8, rng) for _ in range(B)]).astype(np.float32)
    ref = T.warp_pad(img, w, hc, wc)
    h_pad, w_pad = H // 2, W // 2
    gh, gw = H + h_pad, W + w_pad
    assert ref.shape == (B, gh - 2 * w_pad, gw - 2 * h_pad, C)
    dst = guarded.out(ref.shape, F32, DEV)
    ops.tps_warp_pad(inp(img), inp(tps_basis_t(gh, gw, hc, wc)), inp(w), (w_pad, h_pad), (gh, gw), (w_pad, h_pad), dst)
    done()
    got = dst.cpu().numpy()
    mean = float(np.mean(np.abs(got - ref)))
    print('\nTPS WARP PAD %s: max |gpu - oracle| %.3g, mean %.3g' % ((B, H, W, C), float(np.abs(got - ref).max()), mean))
    close_abs(got, ref, 2e-2, 'tps_warp_pad dst')
    assert mean < 3e-4


# ----------------------------------------------------------------------------------------------------------------------------
# C. imm_align_warp_u8, exact in both source modes; D. from tight photo buffers
# ----------------------------------------------------------------------------------------------------------------------------
def run_align(ops, source, owner, geom, coef, basis_t, So, ld):
    """source: ('padded' | 'tight', photos) or ('f32', tensor [n, S, S, 3]).  ld = 3: a dense dst; ld = 4: channels 1..3 of a 4-wide
    stack, whose channel 0 must stay untouched."""
    n = len(owner)
    mode, images = source
    if mode == 'f32':
        src, offs, hw, boxes = inp(images), None, None, None
    else:
        buf, o, shapes = D.PACKERS[mode](images)
        src, offs, hw = inp(buf), inp(o), inp(shapes)
        rows = np.zeros((n, 5), np.int32)                    # only the image index of a box row is read by the warp
        rows[:, 0], rows[:, 3:] = owner, 1
        boxes = inp(rows)
    stack = guarded.out((n, So, So, ld), F32, DEV)
    dst = stack[..., ld - 3:]
    ops.align_warp_u8(src, offs, hw, boxes, inp(geom), inp(coef), None if basis_t is None else inp(basis_t), S, dst)
    done()
    assert untouched(stack[..., :ld - 3]), 'channel 0 of the stack was written'
    return dst.cpu().numpy()


@pytest.mark.parametrize('carrier', ['affine', 'tps'])
@pytest.mark.parametrize('mode', ['padded', 'tight', 'f32'])
@pytest.mark.parametrize('So', D.ALIGN_SO)
def test_align_warp_exact(ops, So, mode, carrier):
    """Shifts by multiples of 4 crop pixels, flips, sub-samplings and box offsets: every source coordinate is an integer, the output
    the indexed photo pixel with exact zeros outside, in the m3 = 3 and the BASIS instantiation (a tps set whose radial rows are 0)."""
    from imm_amd import alignment as AL
    owner, geom, coef, rows, cols = D.align_exact_maps(So)
    images = D.align_f32_sources() if mode == 'f32' else D.align_photos()
    own = np.arange(len(owner)) if mode == 'f32' else owner
    t = R.jittered_grid_template(D.ALIGN_K, 6)
    basis_t = None
    if carrier == 'tps':
        coef = D.as_tps_coef(coef)
        basis_t = AL.LandmarkTemplate(t, S).basis('tps', So).astype(np.float32)
    ref = R.warp(list(images), own, geom, coef, t, S, So)
    _expect, inside = D.align_expect(list(images), own, rows, cols)
    assert 1.0 - inside.mean() >= 0.10 and inside.mean() >= 0.30 and not ref[~inside].any() and ref[inside].all()
    for ld in (3, 4):
        got = run_align(ops, (mode, images), own, geom, coef, basis_t, So, ld)
        np.testing.assert_array_equal(got, ref, err_msg='ld_dst = %d' % ld)


@pytest.mark.parametrize('model', ['similarity', 'tps'])
def test_align_warp_so50_against_f64(ops, model):
    """So = 50: 2500 pixels are no multiple of the 256-thread block and q_step = 2 / 50 is not dyadic.  Landmarks as
    tests/test_alignment_gpu.py test_align_warp_against_f64 draws them; coefficients from the f64 fit, rounded to f32 for both sides."""
    from imm_amd import alignment as AL
    from imm_amd import keypoints as KP
    K, So = 10, 50
    ims = [R.smooth_photo(h, w, 10 + i) for i, (h, w) in enumerate(ALIGN_BOX_PHOTOS)]
    rows = KP.check_boxes(ALIGN_BOXES, len(ims))
    geom = KP.box_geometry(rows, S)
    t = R.jittered_grid_template(K, 3)
    rng = np.random.RandomState(So)
    coef = []
    for _ in rows:
        th, s = rng.uniform(-0.5, 0.5), rng.uniform(0.6, 1.2)
        rot = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        coef.append(R.fit(t, t @ rot.T + rng.uniform(-0.2, 0.2, 2) + rng.standard_normal(t.shape) * 0.04, model))
    coef = np.stack(coef).astype(np.float32)
    basis_t = AL.LandmarkTemplate(t, S).basis('tps', So).astype(np.float32) if model == 'tps' else None
    ref = R.warp(ims, rows[:, 0], geom, coef, t, S, So)
    buf, offs, hw = D.pack_padded(ims)
    dst = guarded.out((len(rows), So, So, 3), F32, DEV)
    ops.align_warp_u8(inp(buf), inp(offs), inp(hw), inp(rows), inp(geom), inp(coef), None if basis_t is None else inp(basis_t), S, dst)
    done()
    got = dst.cpu().numpy()
    print('\nALIGN WARP So=50 %s: max |gpu - f64| %.3g grey levels' % (model, float(np.abs(got - ref).max())))
    close_abs(got, ref, warp_bound(coef.shape[1]), 'align_warp So=50 %s' % model)
    outside = R.wholly_outside(ims, rows[:, 0], geom, coef, t, S, So)
    assert outside[7].all() and outside.sum() > outside[7].sum() and not got[outside].any()


# ----------------------------------------------------------------------------------------------------------------------------
# D. imm_resize_crop_u8 from padded and from tight, guard-flush photo buffers
# ----------------------------------------------------------------------------------------------------------------------------
def small_photos(sizes, c, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 64, size=(h, w, c)).astype(np.uint8) for h, w in sizes]


RESIZE_CASES = [
    # (sizes, c, resize (h, w), margin, final (h, w)); the 31 x 47 photo last
    pytest.param([(218, 178), (200, 160), (1024, 1024), (64, 300), (31, 47)], 3, (160, 160), 16, (128, 128), id='celeba'),
    pytest.param([(33, 47), (2, 2), (1, 5), (31, 47)], 4, (17, 17), 3, (11, 11), id='odd'),
    # down-sizing by exactly 4, 3 and 2: the last output row and column land on the last source row and column
    pytest.param(D.FLUSH_SIZES[0::2], 3, D.FLUSH_RESIZE, 0, D.FLUSH_RESIZE, id='downsize_flush'),
    pytest.param(D.FLUSH_SIZES[1:], 1, D.FLUSH_RESIZE, 0, D.FLUSH_RESIZE, id='downsize_flush_grey'),
]


@pytest.mark.parametrize('packing', ['padded', 'tight'])
@pytest.mark.parametrize('sizes,c,resize,margin,final', RESIZE_CASES)
def test_resize_crop_bit_exact_guarded(ops, sizes, c, resize, margin, final, packing):
    imgs = small_photos(sizes, c, len(sizes))
    buf, offs, hw = D.PACKERS[packing](imgs)
    for ld in (c, c + 1):                                    # ld_dst > c: written at channel 1 of a wider stack
        stack = guarded.out((len(imgs), final[0], final[1], ld), F32, DEV)
        dst = stack[..., ld - c:]
        ops.resize_crop_u8(inp(buf), inp(offs), inp(hw), c, resize, (margin, margin), final, dst)
        done()
        assert untouched(stack[..., :ld - c]), 'channel 0 of the stack was written'
        got = dst.cpu().numpy()
        for i, im in enumerate(imgs):
            want = IO.resize_bilinear(im, resize[0], resize[1])[margin:margin + final[0], margin:margin + final[1]]
            np.testing.assert_array_equal(got[i], want, err_msg='image %d, ld_dst = %d' % (i, ld))


# the box list of tests/test_keypoints_gpu.py test_box_crop_mode_bit_exact, and three boxes on the 31 x 47 photo that ends the buffer
BOX_PHOTOS = [(218, 178), (90, 200), (300, 250), (31, 47)]
BOX_ROWS = [(0, 30, 20, 190, 160), (0, -40, 10, 100, 150), (0, 150, 10, 260, 150), (1, 10, -60, 80, 90), (1, 5, 120, 85, 260),
            (2, -30, -30, 330, 280), (2, 400, 300, 500, 420), (2, 50, 70, 180, 71), (0, 100, 80, 101, 140), (2, 0, 0, 300, 250),
            (2, 100, 60, 227, 187), (2, 7, 9, 20, 11), (3, 0, 0, 31, 47), (3, -10, -10, 40, 60), (3, 5, 7, 20, 30)]


@pytest.mark.parametrize('packing', ['padded', 'tight'])
def test_box_crop_mode_bit_exact_guarded(ops, packing):
    from imm_amd.keypoints import check_boxes
    ims = small_photos(BOX_PHOTOS, 3, 0)
    rows = check_boxes(BOX_ROWS, len(ims))
    buf, offs, hw = D.PACKERS[packing](ims)
    So = 64
    for ld in (3, 4):
        stack = guarded.out((len(rows), So, So, ld), F32, DEV)
        dst = stack[..., ld - 3:]
        ops.resize_crop_u8(inp(buf), inp(offs), inp(hw), 3, (So, So), (0, 0), (So, So), dst, boxes=inp(rows))
        done()
        assert untouched(stack[..., :ld - 3]), 'channel 0 of the stack was written'
        got = dst.cpu().numpy()
        for b, (i, y0, x0, y1, x1) in enumerate(rows):
            ref = IO.resize_bilinear(crop_to_box(ims[i], (y0, x0, y1, x1)), So, So)
            np.testing.assert_array_equal(got[b], ref, err_msg='box %d, ld_dst = %d' % (b, ld))
    assert not got[6].any()                                  # the box outside its image


# ----------------------------------------------------------------------------------------------------------------------------
# E. the keypoint epilogue and imm_align_coeffs under guards
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('K,M', [(10, 5), (64, 16)])
def test_pose_head_keypoint_epilogue_guarded(ops, K, M, dt):
    """tests/test_keypoints_gpu.py test_pose_head_keypoint_epilogue at B = 13 (no multiple of any tile), every output and operand
    guarded: heat, mu, py, px and the maps are the same bits with and without the descriptor, kp is the f64 restatement within
    KP_BOUND."""
    B, C, s, mode = 13, 64, 16, 'rot'
    inv_std, ldh, ldg = 10.0, ops.round_up(K, 4), ops.round_up(K, 8)
    g = torch.Generator().manual_seed(K * 100 + M)
    feat = guarded.inp(torch.randn(B, 16, 16, C, generator=g).to(dt), DEV)
    w = (torch.randn(1, 1, C, K, generator=g) * 0.3).to(DEV)
    bias = guarded.inp(torch.randn(K, generator=g) * 0.5, DEV)
    wt = guarded.out((ops.round_up(K, 128), C), dt, DEV, fill=0)
    ops.pack_weights(w, wt, 0, 1, 1, C, K, C, wt.shape[0], C)
    rng = np.random.RandomState(K + M)
    W = (rng.standard_normal((2 * K, 2 * M)) * 0.3).astype(np.float32)
    bb = (rng.standard_normal(2 * M) * 20).astype(np.float32)
    geom = np.stack([rng.uniform(-50, 300, B), rng.uniform(-50, 300, B), rng.uniform(0.01, 2.4, B), rng.uniform(0.01, 2.4, B)],
                    1).astype(np.float32)
    W_d, bb_d, geom_d = inp(W), inp(bb), inp(geom)
    outs = []
    for with_kp in (False, True):
        heat = guarded.out((B, 16, 16, ldh), F32, DEV)
        mu = guarded.out((B, K, 2), F32, DEV)
        py, px = guarded.out((B, 16, K), F32, DEV), guarded.out((B, 16, K), F32, DEV)
        gauss = guarded.out((B, s, s, ldg), dt, DEV)
        kp = guarded.out((B, M, 2), F32, DEV)
        desc = ops.keypoint_desc(W_d, bb_d, geom_d, kp, S) if with_kp else None
        ops.pose_head_fwd(feat, C, C, wt, bias, B, 16, 16, K, inv_std, s, heat, ldh, mu, py, px, gauss, ldg, dt, mode, keypoints=desc)
        done()
        outs.append((heat[..., :K], mu, py, px, gauss[..., :K], kp))
        if not with_kp:
            assert untouched(kp)
    for name, a, b in zip(('heat', 'mu', 'py', 'px', 'gauss'), outs[0][:5], outs[1][:5]):
        assert bool(torch.isfinite(a.float()).all()), '%s holds an element that is not finite (NaN: never written)' % name
        assert torch.equal(a, b), '%s differs with the keypoint descriptor' % name
    kp = outs[1][5].double().cpu()
    ref = restate(outs[1][1], W, bb, geom, S)
    print('\nKEYPOINT EPILOGUE guarded K=%d M=%d %s: max|kp - f64| %.3g px' % (K, M, dt, float(np.abs(kp.numpy() - ref).max())))
    close_abs(kp, ref, KP_BOUND, 'kp')


@pytest.mark.parametrize('K', [1, 64])
@pytest.mark.parametrize('m3', [3, 67])
def test_align_coeffs_exact(ops, K, m3):
    """Integer mu and F^T in [-3, 3]: every product and every partial sum of the fma chain is an integer below 2 K * 9 <= 1152, exact
    in f32 in any order, so coef equals the integer matrix product bit for bit (the 192-thread block at r2 = 6 and r2 = 134)."""
    n = 5
    rng = np.random.RandomState(10 * K + m3)
    mu = rng.randint(-3, 4, size=(n, K, 2))
    ft = rng.randint(-3, 4, size=(2 * K, 2 * m3))
    want = (mu.reshape(n, 2 * K) @ ft).reshape(n, m3, 2)
    assert int((np.abs(mu.reshape(n, 2 * K)) @ np.abs(ft)).max()) <= 2 * K * 9
    coef = guarded.out((n, m3, 2), F32, DEV)
    ops.align_coeffs(inp(mu.astype(np.float32)), inp(ft.astype(np.float32)), K, m3, coef)
    done()
    np.testing.assert_array_equal(coef.cpu().numpy(), want.astype(np.float32))


# ----------------------------------------------------------------------------------------------------------------------------
# F. the wrappers refuse malformed calls before any launch
# ----------------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_malformed_calls(ops):
    from imm_amd._lib import ImmHipError
    calls = D.refused_calls(ops, DEV)
    for name, call in calls:
        with pytest.raises(ValueError):
            call()
            pytest.fail('%s: accepted' % name)
    done()                                                    # nothing was launched into any of the buffers
    # the library's own refusals stay the library's: c out of range, a crop window outside the resized image
    z = lambda *sh, dtype=F32: guarded.out(sh, dtype, DEV, fill=0)                               # noqa: E731
    with pytest.raises(ImmHipError):
        ops.tps_warp(z(2, 6, 5, 9), z(12, 30), z(2, 12, 2), z(2, 6, 5, 9))
    with pytest.raises(ImmHipError):
        ops.resize_crop_u8(z(96, dtype=torch.uint8), z(2, dtype=torch.int64), z(2, 2, dtype=torch.int32), 5, (6, 6), (1, 1), (4, 4),
                           z(2, 4, 4, 5))
    with pytest.raises(ImmHipError):
        ops.resize_crop_u8(z(96, dtype=torch.uint8), z(2, dtype=torch.int64), z(2, 2, dtype=torch.int32), 3, (6, 6), (3, 3), (4, 4),
                           z(2, 4, 4, 3))
    done()
