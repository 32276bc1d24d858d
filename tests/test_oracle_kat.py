"""Known-answer tests that pin the TF1 semantics (S1..S12) the oracle restates.

The reference ships no tests and TF cannot run here, so every expected value below
is derived by hand from the TF 1.10 op definitions cited in oracle/imm_oracle.py, and the torch
oracle is also cross-checked against the independent fp64 loop code in oracle/np_ref.py.
"""
import math

import numpy as np
import pytest
import torch

from oracle import imm_oracle as O
from oracle import np_ref as R


def t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32))


# ---- S1: SAME padding ----------------------------------------------------------------------
def test_same_pad_formula():
    assert O.same_pad(128, 3, 1) == (1, 1, 128)
    assert O.same_pad(128, 7, 1) == (3, 3, 128)
    assert O.same_pad(128, 3, 2) == (0, 1, 64)      # extra pixel bottom/right, none top/left
    assert O.same_pad(16, 1, 1) == (0, 0, 16)
    assert O.same_pad(5, 3, 2) == (1, 1, 3)


def test_stride2_same_alignment_delta():
    # delta image at (0,0), delta kernel at tap (0,0): with pad_top=0 the output (0,0) sees input (0,0)
    x = torch.zeros(1, 4, 4, 1); x[0, 0, 0, 0] = 1.0
    w = torch.zeros(3, 3, 1, 1); w[0, 0, 0, 0] = 1.0
    y = O.conv2d_same(x, w, None, stride=2)
    assert y.shape == (1, 2, 2, 1)
    assert y[0, 0, 0, 0] == 1.0 and y.sum() == 1.0
    # centre tap (1,1) reads input (2*oy+1, 2*ox+1): a delta at (1,1) lands on output (0,0)
    x = torch.zeros(1, 4, 4, 1); x[0, 1, 1, 0] = 1.0
    w = torch.zeros(3, 3, 1, 1); w[1, 1, 0, 0] = 1.0
    y = O.conv2d_same(x, w, None, stride=2)
    assert y[0, 0, 0, 0] == 1.0 and y.sum() == 1.0
    # PyTorch padding=1 would instead need the delta at (0,0) for the centre tap -> must differ
    x = torch.zeros(1, 4, 4, 1); x[0, 0, 0, 0] = 1.0
    assert O.conv2d_same(x, w, None, stride=2).sum() == 0.0


def test_conv_is_cross_correlation():
    x = torch.zeros(1, 5, 5, 1); x[0, 2, 2, 0] = 1.0
    w = torch.arange(9, dtype=torch.float32).reshape(3, 3, 1, 1)
    y = O.conv2d_same(x, w)[0, :, :, 0]
    # out[oy,ox] = sum w[ky,kx] x[oy+ky-1, ox+kx-1] -> the kernel appears flipped around the delta
    assert y[1, 1] == 8.0 and y[3, 3] == 0.0 and y[2, 2] == 4.0 and y[1, 3] == 6.0


@pytest.mark.parametrize('k,s,h', [(3, 1, 6), (3, 2, 6), (7, 1, 9), (1, 1, 4), (3, 2, 7)])
def test_conv_vs_numpy_loops(k, s, h):
    rng = np.random.default_rng(k * 10 + s)
    x = rng.standard_normal((2, h, h, 3)).astype(np.float32)
    w = rng.standard_normal((k, k, 3, 4)).astype(np.float32)
    b = rng.standard_normal(4).astype(np.float32)
    y = O.conv2d_same(t(x), t(w), t(b), s).numpy()
    np.testing.assert_allclose(y, R.conv2d_same(x, w, b, s), rtol=1e-5, atol=1e-5)


# ---- S2 / S3: resize ------------------------------------------------------------------------
def test_legacy_upsample2x_ramp():
    x = t([0., 1., 2., 3.]).reshape(1, 1, 4, 1).repeat(1, 4, 1, 1)
    y = O.resize_bilinear(x, 8, 8)[0, 0, :, 0]
    # out[2i]=in[i], out[2i+1]=(in[i]+in[min(i+1,n-1)])/2  (no half-pixel offset; last sample repeats)
    np.testing.assert_allclose(y.numpy(), [0, .5, 1, 1.5, 2, 2.5, 3, 3], atol=1e-7)
    # F.interpolate(align_corners=False) uses half-pixel centres and gives [0,.25,.75,...]: must differ
    z = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode='bilinear',
                                        align_corners=False)[0, 0, 0]
    assert abs(float(z[1]) - 0.25) < 1e-6 and abs(float(y[1]) - 0.5) < 1e-7


def test_legacy_downsample_is_strided_pick():
    m = O.smooth_mask(128, 128).reshape(1, 128, 128, 1)
    for s in (128, 64, 32, 16, 8):
        r = 128 // s
        np.testing.assert_array_equal(O.loss_mask_at(m, s).numpy(), m[:, ::r, ::r].numpy())


def test_align_corners_resize():
    x = t([0., 1., 2., 3.]).reshape(1, 4, 1, 1).repeat(1, 1, 4, 1)
    y = O.resize_bilinear(x, 2, 2, align_corners=True)[0, :, 0, 0]
    np.testing.assert_allclose(y.numpy(), [0., 3.], atol=1e-7)   # src = dst*(in-1)/(out-1)
    x32 = torch.arange(32, dtype=torch.float32).reshape(1, 32, 1, 1).repeat(1, 1, 32, 1)
    y16 = O.resize_bilinear(x32, 16, 16, align_corners=True)[0, :, 0, 0]
    np.testing.assert_allclose(y16.numpy(), np.arange(16) * 31.0 / 15.0, rtol=1e-6)


@pytest.mark.parametrize('ac', [False, True])
def test_resize_vs_numpy_loops(ac):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 4, 4, 3)).astype(np.float32)
    np.testing.assert_allclose(O.resize_bilinear(t(x), 8, 8, ac).numpy(), R.resize_bilinear(x, 8, 8, ac),
                               rtol=1e-6, atol=1e-6)
    x = rng.standard_normal((1, 8, 8, 2)).astype(np.float32)
    np.testing.assert_allclose(O.resize_bilinear(t(x), 4, 4, ac).numpy(), R.resize_bilinear(x, 4, 4, ac),
                               rtol=1e-6, atol=1e-6)


# ---- S4: batch norm --------------------------------------------------------------------------
def test_batch_norm_biased_unbiased():
    x = t([1., 2., 3., 6.]).reshape(4, 1, 1, 1)
    y, (mm, mv) = O.batch_norm(x, torch.ones(1), torch.zeros(1), torch.zeros(1), torch.ones(1), True)
    mean, var = 3.0, (4 + 1 + 0 + 9) / 4.0          # biased 3.5
    np.testing.assert_allclose(y.flatten().numpy(), (np.array([1, 2, 3, 6.]) - mean) / math.sqrt(var + 1e-3),
                               rtol=1e-6)
    assert abs(float(mm) - 0.01 * mean) < 1e-7                      # 0*0.99 + 3*0.01
    assert abs(float(mv) - (0.99 + 0.01 * var * 4 / 3)) < 1e-6      # unbiased into the moving average
    ye, (mm2, mv2) = O.batch_norm(x, torch.ones(1), torch.zeros(1), mm, mv, False)
    np.testing.assert_allclose(ye.flatten().numpy(), (np.array([1, 2, 3, 6.]) - float(mm)) / math.sqrt(float(mv) + 1e-3),
                               rtol=1e-6)
    assert mm2 is mm and mv2 is mv


def test_batch_norm_vs_numpy():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 3, 3, 5)).astype(np.float32) * 3 + 1
    g = rng.standard_normal(5).astype(np.float32); b = rng.standard_normal(5).astype(np.float32)
    y, (mm, mv) = O.batch_norm(t(x), t(g), t(b), torch.zeros(5), torch.ones(5), True)
    yr, mean, var, unb = R.batch_norm_train(x, g, b)
    np.testing.assert_allclose(y.numpy(), yr, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(mv.numpy(), 0.99 + 0.01 * unb, rtol=1e-5)


# ---- S7: soft-argmax / gaussians --------------------------------------------------------------
def test_softargmax_uniform_and_peak():
    mu, py, px = O.soft_argmax(torch.zeros(2, 16, 16, 3))
    assert float(mu.abs().max()) < 1e-6 and abs(float(py[0, 0, 0]) - 1 / 16) < 1e-7
    h = torch.zeros(1, 16, 16, 1); h[0, 5, 11, 0] = 16 * 200.0   # row/col means = 200 at (5, 11)
    mu, _, _ = O.soft_argmax(h)
    lin = lambda i: -1 + 2 * i / 15
    assert abs(float(mu[0, 0, 0]) - lin(5)) < 1e-5 and abs(float(mu[0, 0, 1]) - lin(11)) < 1e-5


def test_softargmax_two_point_closed_form():
    # row means: a at row 0, 0 elsewhere -> p0 = e^a/(e^a+15); mu_y = sum p_i lin_i = (p0-p_rest)*(-1) ...
    a = 2.0
    h = torch.zeros(1, 16, 16, 1); h[0, 0, :, 0] = a
    mu, py, _ = O.soft_argmax(h)
    p0 = math.exp(a) / (math.exp(a) + 15)
    pr = 1 / (math.exp(a) + 15)
    exp_mu = p0 * (-1) + pr * sum(-1 + 2 * i / 15 for i in range(1, 16))
    assert abs(float(py[0, 0, 0]) - p0) < 1e-6 and abs(float(mu[0, 0, 0]) - exp_mu) < 1e-6
    assert abs(float(mu[0, 0, 1])) < 1e-6    # column means are all a/16 -> uniform


def test_gaussian_rot_analytic():
    g = O.gaussian_maps(torch.zeros(1, 1, 2), [16, 16], 10.0, 'rot')[0, :, :, 0]
    for (i, j) in [(0, 0), (7, 8), (15, 3)]:
        yl, xl = -1 + 2 * i / 15, -1 + 2 * j / 15
        assert abs(float(g[i, j]) - math.exp(-100 * (yl * yl + xl * xl))) < 1e-7   # no 1/2 factor
    mu = t([[[0.2, -0.6]]])
    g = O.gaussian_maps(mu, [16, 16], 10.0, 'rot')[0, :, :, 0]
    i, j = 9, 3
    yl, xl = -1 + 2 * i / 15, -1 + 2 * j / 15
    assert abs(float(g[i, j]) - math.exp(-100 * ((yl - .2) ** 2 + (xl + .6) ** 2))) < 1e-6


@pytest.mark.parametrize('mode', ['rot', 'flat', 'ankush'])
def test_gaussian_modes_vs_numpy(mode):
    rng = np.random.default_rng(7)
    mu = rng.uniform(-0.9, 0.9, (2, 3, 2)).astype(np.float32)
    g = O.gaussian_maps(t(mu), [8, 8], 10.0, mode).numpy()
    np.testing.assert_allclose(g, R.gaussian_maps(mu, 8, 10.0, mode), rtol=2e-5, atol=1e-6)
    with pytest.raises(ValueError):
        O.gaussian_maps(t(mu), [8, 8], 10.0, 'nope')


def test_softargmax_vs_numpy():
    rng = np.random.default_rng(11)
    h = (rng.standard_normal((2, 16, 16, 4)) * 3).astype(np.float32)
    mu, py, px = O.soft_argmax(t(h))
    rmu, rpy, rpx = R.soft_argmax(h)
    np.testing.assert_allclose(mu.numpy(), rmu, atol=1e-6)
    np.testing.assert_allclose(py.numpy(), rpy, atol=1e-6)
    np.testing.assert_allclose(px.numpy(), rpx, atol=1e-6)


# ---- S8: max pool ---------------------------------------------------------------------------
def test_max_pool_vs_numpy():
    rng = np.random.default_rng(13)
    x = rng.standard_normal((2, 6, 6, 3)).astype(np.float32)
    np.testing.assert_array_equal(O.max_pool2(t(x)).numpy(), R.max_pool2(x))


# ---- S9: clip + Adam -----------------------------------------------------------------------
def test_clip_by_norm():
    g = t([3., 4.])
    np.testing.assert_allclose(O.clip_by_norm(g, 1.0).numpy(), [0.6, 0.8], rtol=1e-6)
    np.testing.assert_allclose(O.clip_by_norm(g, 10.0).numpy(), [3., 4.], rtol=1e-6)   # below c: untouched
    np.testing.assert_allclose(O.clip_by_norm(g, 1.0).numpy(), R.clip_by_norm(g.numpy(), 1.0), rtol=1e-6)


def test_adam_first_step_epsilon_placement():
    # TF form: p -= lr*sqrt(1-b2)/(1-b1) * m/(sqrt(v)+eps) with m=(1-b1)g, v=(1-b2)g^2 at t=1
    P = {'x/w': t([1.0])}
    opt = O.new_adam_state(P)
    g = 1e-4
    newP = O.adam_apply(P, {'x/w': t([g])}, opt, lr=1e-3)
    m, v = 0.1 * g, 0.001 * g * g
    exp = 1.0 - 1e-3 * math.sqrt(1 - 0.999) / (1 - 0.9) * m / (math.sqrt(v) + 1e-8)
    assert abs(float(newP['x/w']) - exp) < 1e-7   # fp32 parameter
    # the "epsilon-hat" (Kingma) form would give 1 - lr*g/(|g|+eps): differs measurably at g=1e-4..1e-7
    p2, _, _ = R.adam_step(np.array([1.0]), np.array([g]), np.zeros(1), np.zeros(1), 1, 1e-3)
    assert abs(float(p2[0]) - exp) < 1e-12
    assert opt['t'] == 1


def test_learning_rate_staircase():
    assert O.learning_rate(0) == 1e-3 and O.learning_rate(99999) == 1e-3
    assert abs(O.learning_rate(100000) - 0.95e-3) < 1e-12
    assert abs(O.learning_rate(250000, lr_multiple=2.0) - 2 * 1e-3 * 0.95 ** 2) < 1e-12


# ---- loss pieces ---------------------------------------------------------------------------
def test_smooth_mask_shape_values():
    m = O.smooth_mask(128, 128)
    assert m.shape == (128, 128)
    assert float(m[:10].abs().max()) == 0.0 and float(m[-10:].abs().max()) == 0.0
    assert abs(float(m[64, 64]) - 1.0) < 1e-7
    s = 0.5 + 0.5 * math.tanh(-1.0 / 0.4)
    assert abs(float(m[10, 64]) - s) < 1e-6      # first sample of the up-step
    assert abs(float(m[64, 117]) - s) < 1e-6     # last sample of the down-step (mirrored)


def test_running_avg_gradient_path():
    # loss_k = m/wl with wl = a + 0.01(m-a): d/dm = 1/wl - 0.01 m/wl^2 (no stop_gradient, base_model.py:39-50)
    a = torch.tensor(1.6)
    m = torch.tensor(2.5, requires_grad=True)
    wl = O.exp_running_avg(m, a)
    (m / wl).backward()
    wlv = 1.6 + 0.01 * (2.5 - 1.6)
    assert abs(float(m.grad) - (1 / wlv - 0.01 * 2.5 / wlv ** 2)) < 1e-6


def test_weight_decay_only_on_kernels():
    cfg = O.default_model_config()
    P, S = O.init_params(cfg, 128)
    wl = float(O.weight_decay_loss(P))
    manual = sum(1e-5 * 0.5 * float((v.double() ** 2).sum()) for k, v in P.items() if k.endswith('/w'))
    assert abs(wl - manual) < 1e-9 * max(1, manual)
    assert len(P) == 96 and sum(v.numel() for v in P.values()) == 4138067   # SURVEY §2a op table
    assert max(float(v.abs().max()) for k, v in P.items() if k.endswith('/w')) <= 0.02 + 1e-9  # truncation


def test_param_counts_other_configs():
    for k, n in ((30, 4189287), (50, 4240507)):
        P, _ = O.init_params(O.default_model_config(k), 128)
        assert sum(v.numel() for v in P.values()) == n
    P, _ = O.init_params(O.default_model_config(30), 256)
    assert sum(v.numel() for v in P.values()) == 4201959
    assert O.render_sizes(O.default_model_config(), 128) == [128, 64, 32, 16]
    assert O.render_sizes(O.default_model_config(), 256) == [256, 128, 64, 32, 16]


def test_errors_match_reference_types():
    cfg = O.default_model_config()
    P, S = O.init_params(cfg, 128)
    inp = O.synthetic_inputs(1, 128)
    del inp['mask']
    with pytest.raises(RuntimeError):
        O.forward(P, S, inp, cfg)
    cfg2 = O.Cfg(cfg); cfg2['reconstruction_loss'] = 'huber'
    with pytest.raises(ValueError):
        O.forward(P, S, O.synthetic_inputs(1, 128), cfg2)


# ---- round 5 (VERDICT r4 item 5 iii): the TF-semantics of S1-S4 pinned one level harder, each expectation derived by hand ----------
def test_legacy_resize_on_non_power_of_two_sizes():
    """S2, tf.image.resize_images(align_corners=False), legacy mapping src = dst * (in / out), no half-pixel offset.
    5 -> 10 (x2 on an odd side): out[2i] = in[i], out[2i+1] = (in[i] + in[min(i+1, 4)]) / 2; the last sample repeats.
    5 -> 3 (ratio 5/3): src = 0, 1.6667, 3.3333 -> out = in[0], in[1]/3 + 2 in[2]/3, 2 in[3]/3 + in[4]/3.
    12 -> 4 (integer factor 3, the loss-mask case at a non-power-of-two side): src = 0, 3, 6, 9 -> a strided pick."""
    v = np.array([1., 4., 9., 16., 25.], np.float32)                      # in[i] = (i + 1)^2: not linear, so the weights show
    x = t(v).reshape(1, 1, 5, 1)
    np.testing.assert_allclose(O.resize_bilinear(x, 1, 10)[0, 0, :, 0].numpy(),
                               [1, 2.5, 4, 6.5, 9, 12.5, 16, 20.5, 25, 25], atol=1e-6)
    np.testing.assert_allclose(O.resize_bilinear(x, 1, 3)[0, 0, :, 0].numpy(),
                               [1.0, 4. / 3 + 2 * 9. / 3, 2 * 16. / 3 + 25. / 3], rtol=1e-6)
    r = np.arange(12, dtype=np.float32) ** 2
    y = O.resize_bilinear(t(r).reshape(1, 12, 1, 1).repeat(1, 1, 12, 1), 4, 4)
    np.testing.assert_array_equal(y[0, :, 0, 0].numpy(), r[::3])
    np.testing.assert_array_equal(y[0, 0, :, 0].numpy(), np.full(4, r[0]))    # columns: constant rows stay constant
    # both axes at once on a 2-D ramp f(y, x) = 10 y + x, 3x5 -> 6x10: separable, rows then columns give the same as the closed form
    g = (10 * np.arange(3, dtype=np.float32)[:, None] + np.arange(5, dtype=np.float32)[None]).reshape(1, 3, 5, 1)
    got = O.resize_bilinear(t(g), 6, 10)[0, :, :, 0].numpy()
    ry = np.array([0, .5, 1, 1.5, 2, 2]); rx = np.array([0, .5, 1, 1.5, 2, 2.5, 3, 3.5, 4, 4])
    np.testing.assert_allclose(got, 10 * ry[:, None] + rx[None], atol=1e-6)


def test_align_corners_resize_on_non_power_of_two_sizes():
    """S3, tf.image.resize_bilinear(align_corners=True): src = dst * (in - 1) / (out - 1).
    5 -> 3: src = 0, 2, 4 (exact picks).  4 -> 7: src = 0, .5, 1, ... -> midpoints in between.  6 -> 4: src = 0, 5/3, 10/3, 5 ->
    out[1] = in[1]/3 + 2 in[2]/3, out[2] = 2 in[3]/3 + in[4]/3.  (S = 96 would resize 12 -> 16 with (in-1)/(out-1) = 11/15.)"""
    v5 = np.array([1., 4., 9., 16., 25.], np.float32)
    np.testing.assert_allclose(O.resize_bilinear(t(v5).reshape(1, 5, 1, 1), 3, 1, True)[0, :, 0, 0].numpy(), [1, 9, 25], atol=1e-6)
    v4 = np.array([1., 4., 9., 16.], np.float32)
    np.testing.assert_allclose(O.resize_bilinear(t(v4).reshape(1, 4, 1, 1), 7, 1, True)[0, :, 0, 0].numpy(),
                               [1, 2.5, 4, 6.5, 9, 12.5, 16], atol=1e-6)
    v6 = np.array([1., 4., 9., 16., 25., 36.], np.float32)
    np.testing.assert_allclose(O.resize_bilinear(t(v6).reshape(1, 1, 6, 1), 1, 4, True)[0, 0, :, 0].numpy(),
                               [1, 4. / 3 + 2 * 9. / 3, 2 * 16. / 3 + 25. / 3, 36], rtol=1e-6)
    v12 = np.arange(12, dtype=np.float32)
    got = O.resize_bilinear(t(v12).reshape(1, 12, 1, 1), 16, 1, True)[0, :, 0, 0].numpy()
    np.testing.assert_allclose(got, np.arange(16) * 11.0 / 15.0, rtol=1e-6, atol=1e-6)         # a ramp maps to a ramp


def test_batch_norm_with_batch_one_uses_the_spatial_positions():
    """S4 at batch 1 (the K=30 golden case runs at batch 1): the statistics are over N*H*W = 4 positions of the ONE image —
    x = [[1, 2], [3, 6]]: mean 3, biased variance (4 + 1 + 0 + 9) / 4 = 3.5 normalises, the unbiased 14/3 enters the moving
    variance (momentum 0.99), eps 1e-3; gamma 2 / beta -1 scale and shift AFTER the normalisation."""
    x = t([[1., 2.], [3., 6.]]).reshape(1, 2, 2, 1)
    y, (mm, mv) = O.batch_norm(x, torch.full((1,), 2.0), torch.full((1,), -1.0), torch.zeros(1), torch.ones(1), True)
    want = (np.array([[1, 2], [3, 6.]]) - 3.0) / math.sqrt(3.5 + 1e-3) * 2.0 - 1.0
    np.testing.assert_allclose(y[0, :, :, 0].numpy(), want, rtol=1e-6)
    assert abs(float(mm) - 0.03) < 1e-7 and abs(float(mv) - (0.99 + 0.01 * 14.0 / 3.0)) < 1e-6
    # a single position (n = 1): variance 0, output = beta, and the unbiased factor n / max(n - 1, 1) stays finite
    y1, (_m, mv1) = O.batch_norm(t([5.]).reshape(1, 1, 1, 1), torch.ones(1), torch.full((1,), 0.25), torch.zeros(1), torch.ones(1), True)
    assert abs(float(y1) - 0.25) < 1e-7 and abs(float(mv1) - 0.99) < 1e-7


def test_conv7_same_padding_on_odd_and_even_sides():
    """S1 for the 7x7 first convolution (imm_model.py:190), delta image through an index kernel w[ky][kx] = 7 ky + kx:
    stride 1, side 5 (odd): pad 3 | 3, out[y][x] = w[5 - y][5 - x] for a delta at (2, 2);
    stride 2, side 5 -> 3: pad_total = (3-1)*2 + 7 - 5 = 6 -> 3 | 3, out[oy][ox] = w[5 - 2 oy][5 - 2 ox];
    stride 2, side 6 -> 3 (even): pad_total = 5 -> 2 before, 3 after, out[oy][ox] = w[4 - 2 oy][4 - 2 ox]."""
    w = torch.arange(49, dtype=torch.float32).reshape(7, 7, 1, 1)
    x5 = torch.zeros(1, 5, 5, 1); x5[0, 2, 2, 0] = 1.0
    y = O.conv2d_same(x5, w)[0, :, :, 0].numpy()
    assert y.shape == (5, 5)
    for yy in range(5):
        for xx in range(5):
            assert y[yy, xx] == 7 * (5 - yy) + (5 - xx)
    assert O.same_pad(5, 7, 1) == (3, 3, 5) and O.same_pad(5, 7, 2) == (3, 3, 3) and O.same_pad(6, 7, 2) == (2, 3, 3)
    y2 = O.conv2d_same(x5, w, None, 2)[0, :, :, 0].numpy()
    np.testing.assert_array_equal(y2, [[7 * (5 - 2 * a) + (5 - 2 * b) for b in range(3)] for a in range(3)])
    x6 = torch.zeros(1, 6, 6, 1); x6[0, 2, 2, 0] = 1.0
    y3 = O.conv2d_same(x6, w, None, 2)[0, :, :, 0].numpy()
    np.testing.assert_array_equal(y3, [[7 * (4 - 2 * a) + (4 - 2 * b) for b in range(3)] for a in range(3)])


def test_cost_moving_average_is_the_biased_tf110_shadow():
    """base_model.py:52-60 under the pinned TF 1.10 (ExponentialMovingAverage(zero_debias=False)): the shadow of a cost TENSOR starts
    at 0 and is NOT debiased — after one step it is 0.01 x1, after two 0.99 * 0.01 x1 + 0.01 x2; a constant cost c reads
    c (1 - 0.99^t) after t steps."""
    st, avg = O.cost_ema_update([0.0, 0.0], [5.0])
    assert abs(avg[0] - 0.05) < 1e-12 and st[1] == 1.0
    st, avg = O.cost_ema_update(st, [7.0])
    assert abs(avg[0] - (0.99 * 0.01 * 5.0 + 0.01 * 7.0)) < 1e-12
    st = [0.0, 0.0]
    for _ in range(50):
        st, avg = O.cost_ema_update(st, [3.25])
    assert abs(avg[0] - 3.25 * (1 - 0.99 ** 50)) < 1e-9


# ---- non-square maps: the oracle at the shapes tests/test_geometry_gpu.py leans on, against direct f64 loops ----------------------
# Each loop below is written from the TF 1.10 op definition (not from oracle/np_ref.py, whose helpers are square-only in places):
# height and width are never interchangeable in them, so an oracle that used the wrong extent on one axis cannot agree.
def _conv_same_loops(x, w, b, s):
    """tf.nn.conv2d SAME: per axis n_out = ceil(n/s), pad_total = max((n_out-1)*s + k - n, 0), pad_before = pad_total // 2."""
    B, H, W, Ci = x.shape
    kh, kw, _, Co = w.shape
    ho, wo = -(-H // s), -(-W // s)
    pt = max((ho - 1) * s + kh - H, 0) // 2
    pl = max((wo - 1) * s + kw - W, 0) // 2
    y = np.zeros((B, ho, wo, Co), np.float64)
    for oy in range(ho):
        for ox in range(wo):
            for ky in range(kh):
                iy = oy * s + ky - pt
                if iy < 0 or iy >= H:
                    continue
                for kx in range(kw):
                    ix = ox * s + kx - pl
                    if ix < 0 or ix >= W:
                        continue
                    y[:, oy, ox] += x[:, iy, ix].astype(np.float64) @ w[ky, kx].astype(np.float64)
    return y + (0 if b is None else b.astype(np.float64))


def _resize_loops(x, oh, ow, ac):
    """tf.image.resize_bilinear: src = dst * (in-1)/(out-1) with align_corners (out > 1), else dst * in/out; lo = floor(src),
    hi = min(lo + 1, in - 1); columns are interpolated within the top and the bottom row, then the rows."""
    B, H, W, C = x.shape
    sy = (H - 1) / (oh - 1) if ac and oh > 1 else H / oh
    sx = (W - 1) / (ow - 1) if ac and ow > 1 else W / ow
    y = np.zeros((B, oh, ow, C), np.float64)
    xd = x.astype(np.float64)
    for Y in range(oh):
        fy = Y * sy
        y0 = int(math.floor(fy)); y1 = min(y0 + 1, H - 1); ly = fy - y0
        for X in range(ow):
            fx = X * sx
            x0 = int(math.floor(fx)); x1 = min(x0 + 1, W - 1); lx = fx - x0
            top = xd[:, y0, x0] + (xd[:, y0, x1] - xd[:, y0, x0]) * lx
            bot = xd[:, y1, x0] + (xd[:, y1, x1] - xd[:, y1, x0]) * lx
            y[:, Y, X] = top + (bot - top) * ly
    return y


@pytest.mark.parametrize('k,s,h,w', [(3, 1, 5, 8), (3, 1, 8, 5), (3, 2, 6, 9), (3, 2, 9, 6), (3, 2, 7, 4), (7, 1, 4, 9), (7, 2, 6, 5),
                                     (1, 1, 3, 7)])
def test_conv_same_on_non_square_maps(k, s, h, w):
    """S1 per axis: stride 1 and 2, odd and even sides, tall and wide; the 3 x 2-stride (6, 9) case pads 0|1 rows and 1|1 columns."""
    rng = np.random.default_rng(100 * k + 10 * s + h)
    x = rng.standard_normal((2, h, w, 3)).astype(np.float32)
    wt = rng.standard_normal((k, k, 3, 4)).astype(np.float32)
    b = rng.standard_normal(4).astype(np.float32)
    y = O.conv2d_same(t(x), t(wt), t(b), s).numpy()
    assert y.shape == (2, -(-h // s), -(-w // s), 4)
    np.testing.assert_allclose(y, _conv_same_loops(x, wt, b, s), rtol=1e-5, atol=1e-5)


def test_conv_same_non_square_kernel_and_delta():
    """A 7x1 kernel (the tap-unrolled first layer) pads rows only; a delta at (1, 4) of a 4x6 map through an index kernel."""
    rng = np.random.default_rng(17)
    x = rng.standard_normal((1, 6, 10, 2)).astype(np.float32)
    wt = rng.standard_normal((7, 1, 2, 3)).astype(np.float32)
    np.testing.assert_allclose(O.conv2d_same(t(x), t(wt)).numpy(), _conv_same_loops(x, wt, None, 1), rtol=1e-5, atol=1e-5)
    d = torch.zeros(1, 4, 6, 1); d[0, 1, 4, 0] = 1.0
    w9 = torch.arange(9, dtype=torch.float32).reshape(3, 3, 1, 1)
    y = O.conv2d_same(d, w9)[0, :, :, 0]
    # out[oy][ox] = w[1 + 1 - oy][1 + 4 - ox]
    assert y.shape == (4, 6) and y[0, 3] == 8.0 and y[2, 5] == 0.0 and y[1, 4] == 4.0 and y[0, 5] == 6.0 and float(y[3].abs().max()) == 0.0


@pytest.mark.parametrize('ac', [False, True], ids=['legacy', 'align_corners'])
@pytest.mark.parametrize('hw,ohw', [((4, 6), (8, 12)), ((6, 4), (12, 8)), ((8, 12), (4, 6)), ((12, 8), (6, 4)), ((8, 16), (4, 4)),
                                    ((5, 3), (3, 7))])
def test_resize_on_non_square_maps(hw, ohw, ac):
    """S2 / S3 with independent row and column ratios (the (8, 16) -> (4, 4) case: 2 and 4; (5, 3) -> (3, 7): down and up)."""
    rng = np.random.default_rng(hw[0] * 31 + ohw[1])
    x = rng.standard_normal((2, hw[0], hw[1], 3)).astype(np.float32)
    y = O.resize_bilinear(t(x), ohw[0], ohw[1], ac).numpy()
    assert y.shape == (2, ohw[0], ohw[1], 3)
    np.testing.assert_allclose(y, _resize_loops(x, ohw[0], ohw[1], ac), rtol=1e-5, atol=1e-6)


def test_resize_non_square_ramp_closed_form():
    """f(y, x) = 10 y + x on 3 x 5 -> 5 x 9 with align_corners: src_y = Y / 2, src_x = X / 2, a ramp stays a ramp on each axis."""
    g = (10 * np.arange(3, dtype=np.float32)[:, None] + np.arange(5, dtype=np.float32)[None]).reshape(1, 3, 5, 1)
    got = O.resize_bilinear(t(g), 5, 9, True)[0, :, :, 0].numpy()
    np.testing.assert_allclose(got, 10 * (np.arange(5) / 2.0)[:, None] + (np.arange(9) / 2.0)[None], atol=1e-6)


@pytest.mark.parametrize('h,w', [(4, 6), (6, 4), (2, 8)])
def test_max_pool_on_non_square_maps(h, w):
    rng = np.random.default_rng(h * 7 + w)
    x = rng.standard_normal((2, h, w, 3)).astype(np.float32)
    ref = np.zeros((2, h // 2, w // 2, 3), np.float32)
    for Y in range(h // 2):
        for X in range(w // 2):
            ref[:, Y, X] = np.maximum(np.maximum(x[:, 2 * Y, 2 * X], x[:, 2 * Y, 2 * X + 1]),
                                      np.maximum(x[:, 2 * Y + 1, 2 * X], x[:, 2 * Y + 1, 2 * X + 1]))
    got = O.max_pool2(t(x)).numpy()
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize('h,w', [(4, 7), (7, 4), (16, 32)])
def test_softargmax_on_non_square_maps(h, w):
    """imm_model.py:252-264: the row profile is softmax over h of the mean over w (and the other way round), coordinates are
    linspace(-1, 1, h) and linspace(-1, 1, w); py is [B, h, K], px [B, w, K]."""
    rng = np.random.default_rng(h + 3 * w)
    heat = (rng.standard_normal((2, h, w, 3)) * 3).astype(np.float32)
    mu, py, px = O.soft_argmax(t(heat))
    assert mu.shape == (2, 3, 2) and py.shape == (2, h, 3) and px.shape == (2, w, 3)
    hd = heat.astype(np.float64)
    for b in range(2):
        for k in range(3):
            rows = np.array([sum(hd[b, i, j, k] for j in range(w)) / w for i in range(h)])
            cols = np.array([sum(hd[b, i, j, k] for i in range(h)) / h for j in range(w)])
            pr = np.exp(rows - rows.max()); pr /= pr.sum()
            pc = np.exp(cols - cols.max()); pc /= pc.sum()
            np.testing.assert_allclose(py[b, :, k].numpy(), pr, atol=1e-6)
            np.testing.assert_allclose(px[b, :, k].numpy(), pc, atol=1e-6)
            my = sum(pr[i] * (-1 + 2 * i / (h - 1)) for i in range(h))
            mx = sum(pc[j] * (-1 + 2 * j / (w - 1)) for j in range(w))
            assert abs(float(mu[b, k, 0]) - my) < 2e-6 and abs(float(mu[b, k, 1]) - mx) < 2e-6


@pytest.mark.parametrize('mode', ['rot', 'flat', 'ankush'])
@pytest.mark.parametrize('h,w', [(4, 9), (9, 4)])
def test_gaussian_maps_on_non_square_maps(h, w, mode):
    """imm_model.py:34-78 with shape_hw = [h, w]: y runs over linspace(-1, 1, h), x over linspace(-1, 1, w); output [B, h, w, K]."""
    rng = np.random.default_rng(h * 5 + w)
    mu = rng.uniform(-0.9, 0.9, (2, 3, 2)).astype(np.float32)
    g = O.gaussian_maps(t(mu), [h, w], 10.0, mode).numpy()
    assert g.shape == (2, h, w, 3)
    ref = np.zeros((2, h, w, 3), np.float64)
    for b in range(2):
        for k in range(3):
            for i in range(h):
                for j in range(w):
                    dy = float(mu[b, k, 0]) - (-1 + 2 * i / (h - 1)); dx = float(mu[b, k, 1]) - (-1 + 2 * j / (w - 1))
                    if mode == 'rot':
                        ref[b, i, j, k] = math.exp(-(dy * dy + dx * dx) * 100.0)
                    elif mode == 'flat':
                        ref[b, i, j, k] = math.exp(-((dy * dy + dx * dx) * 100.0 + 1e-5) ** 0.25)
                    else:
                        ref[b, i, j, k] = math.exp(-math.sqrt(1e-4 + abs(dy * 10.0))) * math.exp(-math.sqrt(1e-4 + abs(dx * 10.0)))
    np.testing.assert_allclose(g, ref, rtol=2e-5, atol=1e-6)
