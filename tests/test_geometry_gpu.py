"""Kernel parity with the row strides pulled apart from the channel counts (ld > c) and the map height from its width.

Every entry point of libimm_hip.so takes `ld*` separately from `c` and `h` separately from `w`; the engine uses that (the concat
buffer `joint` has two writers that own disjoint columns), tests/test_kernels_gpu.py does not (ld == c, square maps).  Here each
non-convolution entry point runs on
  - inputs embedded in a wider row whose columns [c, ld) are NaN: nothing may read them into a result (close() fails on NaN);
  - outputs whose whole body starts as 0xFF bytes: columns [c, ld) must still be 0xFF afterwards (untouched());
  - maps with h != w, in both orientations (a transposed bug can cancel in one of them),
against the same oracle expression and with the same tolerance as the entry point's test in test_kernels_gpu.py: strides and
aspect ratio change addresses, not arithmetic.  The convolution families are covered beside their tables in test_kernels_gpu.py.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import imm_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded                                                              # noqa: E402
from guarded import close, untouched                                        # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


@pytest.fixture(autouse=True)
def _guards_intact():
    """After every test: no kernel wrote outside a tensor it was handed (tests/guarded.py)."""
    guarded.reset()
    yield
    guarded.check_guards()


def rnd(shape, seed, scale=1.0, dt=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dt)


def wide(x, ld, fill=NAN):
    """A kernel INPUT [..., c] embedded in [..., ld] on the device, between guard bands; the columns [c, ld) hold `fill` (NaN: a
    kernel that reads them into a result fails close())."""
    c = x.shape[-1]
    assert ld >= c
    out = torch.full(tuple(x.shape[:-1]) + (ld,), fill, dtype=x.dtype)
    out[..., :c] = x
    return guarded.inp(out, DEV, depth=2)


def dev(x):
    return guarded.inp(x, DEV, depth=2)


def gout(shape, dt=torch.bfloat16, fill=None):
    return guarded.out(shape, dt, DEV, fill=fill, what=guarded._caller(1))


def vec(n, fill=None):
    return guarded.out((n,), torch.float32, DEV, fill=fill)


# ----------------------------------------------------------------------------------------------
# batch norm: apply / fused apply / backward reduce, apply, fused apply      (A: ldy, ldo, lddo, lddy)
# ----------------------------------------------------------------------------------------------
BN_STRIDES = [
    # c, npix, ldy, ldo, lddo, lddy
    (64, 1000, 72, 80, 88, 96),          # the smallest legal strides, all four different; 1000 pixels: ragged against every block size
    (256, 512, 256, 288, 288, 264),      # the engine's pair: a compact conv output normalised INTO the concat buffer (ldo = Cj) and
                                         # the concat buffer's gradient read back (lddo = Cj)
    (256, 512, 320, 256, 256, 320),      # the other way round (Cj of the 64-channel-slice engines)
    (32, 1000, 40, 32, 32, 40),
    (16, 2048, 24, 32, 40, 24),          # c % 32 != 0: the un-fused entry points only
]


@pytest.mark.parametrize('c,npix,ldy,ldo,lddo,lddy', BN_STRIDES, ids=['c%d_ld%d_%d_%d_%d' % ((t[0],) + t[2:]) for t in BN_STRIDES])
def test_batch_norm_strides(ops, c, npix, ldy, ldo, lddo, lddy):
    """imm_bn_apply_relu, imm_bn_apply_fused, imm_bn_bwd_reduce, imm_bn_bwd_apply, imm_bn_bwd_apply_fused with every stride above the
    channel count: the oracle expressions and tolerances of test_batch_norm_fwd_bwd / test_batch_norm_finalize_fused_into_apply."""
    dt = torch.bfloat16
    y = (rnd((npix, c), 41) * 2 + 0.5).to(dt)
    gamma = rnd((c,), 42, 0.5, torch.float32) + 1.0
    beta = rnd((c,), 43, 0.5, torch.float32)
    yf = y.float()
    partial = dev(torch.stack([yf.sum(0), (yf * yf).sum(0)]).reshape(1, 2, c).contiguous())
    gd, bd = dev(gamma), dev(beta)
    mm, mv = vec(c, 0), vec(c, 1)
    scale, shift, mean, rstd = (vec(c) for _ in range(4))
    ops.bn_finalize(partial, 1, c, npix, gd, bd, 1e-3, 0.99, True, mm, mv, scale, shift, mean, rstd)
    yw = wide(y, ldy)
    xo = gout((npix, ldo))
    ops.bn_apply_relu(yw, npix, c, ldy, scale, shift, True, xo, ldo)
    torch.cuda.synchronize()
    yr = yf.reshape(1, 1, npix, c).clone().requires_grad_(True)
    g_, b_ = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref, _ = O.batch_norm(yr, g_, b_, torch.zeros(c), torch.ones(c), True)
    ref = torch.relu(ref)
    close(xo[:, :c], ref.reshape(npix, c), 1e-2, 2e-3, 'bn_apply_relu')
    assert untouched(xo[:, c:]), 'imm_bn_apply_relu wrote columns [c, ldo) of its output'
    fused = c % 32 == 0
    if fused:
        mm2, mv2 = vec(c, 0), vec(c, 1)
        s2, h2, m2, r2 = (vec(c) for _ in range(4))
        xf = gout((npix, ldo))
        ops.bn_apply_fused(partial, 1, c, npix, gd, bd, 1e-3, 0.99, True, mm2, mv2, s2, h2, m2, r2, yw, ldy, True, xf, ldo)
        torch.cuda.synchronize()
        close(xf[:, :c], ref.reshape(npix, c), 1e-2, 2e-3, 'bn_apply_fused vs oracle')
        close(xf[:, :c], xo[:, :c], 8e-3, 1e-3, 'bn_apply_fused vs finalize + apply')
        for a, b, what in ((mm2, mm, 'moving_mean'), (mv2, mv, 'moving_var'), (s2, scale, 'scale'), (h2, shift, 'shift'),
                           (m2, mean, 'mean'), (r2, rstd, 'rstd')):
            close(a, b, 1e-6, 1e-6, 'bn_apply_fused/' + what)
        assert untouched(xf[:, c:]), 'imm_bn_apply_fused wrote columns [c, ldo) of its output'
    # backward
    dout = rnd((npix, c), 44)
    gy, gg, gb = torch.autograd.grad(ref, [yr, g_, b_], dout.float().reshape(1, 1, npix, c))
    nblk = ops.bn_bwd_blocks(npix, c)
    part = gout((nblk, 2, c), torch.float32)
    dow = wide(dout, lddo)
    ops.bn_bwd_reduce(dow, lddo, yw, ldy, npix, c, scale, shift, mean, rstd, True, part)
    dg, db, coef = vec(c), vec(c), gout((3, c), torch.float32)
    ops.bn_bwd_finalize(part, nblk, c, npix, gd, bd, rstd, dg, db, coef)
    dyo = gout((npix, lddy))
    ops.bn_bwd_apply(dow, lddo, yw, ldy, npix, c, scale, shift, mean, rstd, True, coef, dyo, lddy)
    torch.cuda.synchronize()
    close(dg, gg, 2e-3, 1e-3, 'bn_dgamma')
    close(db, gb, 2e-3, 1e-3, 'bn_dbeta')
    close(dyo[:, :c], gy.reshape(npix, c), 2e-2, 4e-3, 'bn_bwd_apply')
    assert untouched(dyo[:, c:]), 'imm_bn_bwd_apply wrote columns [c, lddy) of its output'
    if fused:
        dg2, db2 = vec(c), vec(c)
        dyf = gout((npix, lddy))
        ops.bn_bwd_apply_fused(part, nblk, c, npix, gd, dow, lddo, yw, ldy, scale, shift, mean, rstd, True, dg2, db2, dyf, lddy)
        torch.cuda.synchronize()
        close(dg2, dg, 1e-6, 1e-6, 'bn_bwd_apply_fused/dgamma'); close(db2, db, 1e-6, 1e-6, 'bn_bwd_apply_fused/dbeta')
        close(dyf[:, :c], gy.reshape(npix, c), 2e-2, 4e-3, 'bn_bwd_apply_fused vs oracle')
        close(dyf[:, :c], dyo[:, :c], 8e-3, 1e-3, 'bn_bwd_apply_fused vs finalize + apply')
        assert untouched(dyf[:, c:]), 'imm_bn_bwd_apply_fused wrote columns [c, lddy) of its output'


def test_batch_norm_fused_rejects_narrow_channel_counts(ops):
    """c = 16 (one of the non-square shapes of the up-sampling kernels) is not a shape of the fused passes: refused, not served."""
    from imm_amd import _lib as L
    c, npix = 16, 64
    v = vec(c, 0)
    y = gout((npix, c), fill=0)
    with pytest.raises(L.ImmHipError, match='bn_apply_fused: C=16 must be a multiple of 32'):
        ops.bn_apply_fused(None, 0, c, npix, v, v, 1e-3, 0.99, False, v, v, v, v, v, v, y, c, True, gout((npix, c)), c)
    part = gout((1, 2, c), torch.float32, fill=0)
    with pytest.raises(L.ImmHipError, match='bn_bwd_apply_fused: C=16 must be a multiple of 32'):
        ops.bn_bwd_apply_fused(part, 1, c, npix, v, y, c, y, c, v, v, v, v, True, v, v, gout((npix, c)), c)
    with pytest.raises(L.ImmHipError, match='must be multiples of 8'):
        ops.bn_apply_relu(y, npix, c, c, v, v, True, gout((npix, 12)), 12)           # ld < c


# ----------------------------------------------------------------------------------------------
# x2 up-sampling and everything fused with it        (A: ldx, ldy, ldo;  B: (8, 24) and (24, 8))
# ----------------------------------------------------------------------------------------------
UP_CASES = [
    # B, h, w, c, ld of the small tensor, ld of the up-sampled tensor, ld of `out` / `y`
    (2, 8, 8, 16, 24, 32, 40),           # the existing small shape, every stride different
    (3, 8, 24, 16, 16, 16, 16),          # wide
    (3, 24, 8, 16, 16, 16, 16),          # tall
    (3, 8, 24, 64, 72, 80, 88),
    (3, 24, 8, 64, 80, 72, 64),
    (5, 10, 20, 64, 64, 72, 72),         # 1000 pixels
]
UP_IDS = ['b%d_%dx%d_c%d_ld%d_%d_%d' % t for t in UP_CASES]


@pytest.mark.parametrize('B,h,w,c,lds,ldu,ldo', UP_CASES, ids=UP_IDS)
def test_upsample2x_strides_and_non_square(ops, B, h, w, c, lds, ldu, ldo):
    """imm_upsample2x_fwd / _bwd against the oracle resize + autograd (test_upsample2x), imm_upsample2x_bwd_bn against the masked
    adjoint and its sums (test_upsample2x_bwd_with_bn_backward_sums), imm_bn_bwd_reduce_up against the two launches it replaces
    (test_bn_bwd_reduce_with_upsampling_adjoint)."""
    dt = torch.bfloat16
    x = rnd((B, h, w, c), 51)
    xr = x.float().requires_grad_(True)
    ref = O.resize_bilinear(xr, 2 * h, 2 * w)
    y = gout((B, 2 * h, 2 * w, ldu))
    ops.upsample2x_fwd(wide(x, lds), y, B, h, w, c, lds, ldu)
    dy = rnd((B, 2 * h, 2 * w, c), 52)
    (gx,) = torch.autograd.grad(ref, xr, dy.float())
    dyw = wide(dy, ldu)
    dx = gout((B, h, w, lds))
    ops.upsample2x_bwd(dyw, dx, B, h, w, c, ldu, lds)
    torch.cuda.synchronize()
    close(y[..., :c], ref, 8e-3, 1e-3, 'upsample_fwd')
    close(dx[..., :c], gx, 8e-3, 2e-3, 'upsample_bwd')
    assert untouched(y[..., c:]) and untouched(dx[..., c:]), 'imm_upsample2x_fwd / _bwd wrote columns [c, ld) of an output'
    # adjoint + ReLU mask + batch-norm backward sums
    out = rnd((B, h, w, c), 55)
    nblk = ops.upsample2x_bwd_bn_blocks(B, h, w, c)
    part = gout((nblk, 2, c), torch.float32)
    dxm = gout((B, h, w, lds))
    ops.upsample2x_bwd_bn(dyw, dxm, B, h, w, c, ldu, lds, wide(out, ldo), ldo, part)
    torch.cuda.synchronize()
    want = dx[..., :c].float().cpu() * (out.float() > 0)
    assert torch.equal(dxm[..., :c].float().cpu(), want)
    assert untouched(dxm[..., c:]), 'imm_upsample2x_bwd_bn wrote columns [c, lddx) of dx'
    s = part.sum(dim=0)
    close(s[0], want.sum(dim=(0, 1, 2)), 5e-3, 5e-3, 'upsample_bwd_bn/sum dz')
    close(s[1], (want * out.float()).sum(dim=(0, 1, 2)), 5e-3, 5e-3, 'upsample_bwd_bn/sum dz*out')
    # adjoint + batch-norm backward reduction
    yb = (rnd((B, h, w, c), 192) * 2 + 0.3).to(dt)
    scale = dev(rnd((c,), 193, 0.3, torch.float32) + 1.0); shift = dev(rnd((c,), 194, 0.5, torch.float32))
    mean = dev(rnd((c,), 195, 0.5, torch.float32)); rstd = dev(rnd((c,), 196, 0.1, torch.float32).abs() + 0.5)
    npix = B * h * w
    nb = ops.bn_bwd_blocks(npix, c)
    d_ref = gout((B, h, w, c)); p_ref = gout((nb, 2, c), torch.float32)
    dyc, ybc = dev(dy), dev(yb)
    ops.upsample2x_bwd(dyc, d_ref, B, h, w, c, c, c)
    ops.bn_bwd_reduce(d_ref, c, ybc, c, npix, c, scale, shift, mean, rstd, True, p_ref)
    d_got = gout((B, h, w, lds)); p_got = gout((nb, 2, c), torch.float32)
    ops.bn_bwd_reduce_up(dyw, ldu, d_got, lds, wide(yb, ldo), ldo, B, h, w, c, scale, shift, mean, rstd, True, p_got)
    torch.cuda.synchronize()
    assert torch.equal(d_ref, dx[..., :c]), 'the compact and the wide adjoint differ'
    assert torch.equal(d_got[..., :c], d_ref) and untouched(d_got[..., c:])
    assert torch.equal(p_got, p_ref), float((p_got - p_ref).abs().max())


UPF_CASES = [(3, 8, 24, 64, 72, 80, 88), (3, 24, 8, 64, 64, 72, 80), (5, 10, 20, 32, 40, 32, 48), (2, 8, 8, 32, 32, 40, 32)]


@pytest.mark.parametrize('B,h,w,c,ldy,ldo,ldu', UPF_CASES, ids=['b%d_%dx%d_c%d_ld%d_%d_%d' % t for t in UPF_CASES])
def test_bn_apply_fused_with_upsampling_strides_and_non_square(ops, B, h, w, c, ldy, ldo, ldu):
    """imm_bn_apply_fused with the renderer's x2 up-sampled output (test_batch_norm_finalize_fused_into_apply): bitwise the separate
    up-sampling kernel applied to the 16-bit normalised tensor, which is itself compared with the oracle."""
    dt = torch.bfloat16
    npix = B * h * w
    y = (rnd((npix, c), 241) * 2 + 0.5).to(dt)
    gamma = dev(rnd((c,), 242, 0.5, torch.float32) + 1.0)
    beta = dev(rnd((c,), 243, 0.5, torch.float32))
    mm, mv = dev(rnd((c,), 244, 0.3, torch.float32) + 0.5), dev(rnd((c,), 245, 0.2, torch.float32).abs() + 1.0)
    s2, h2, m2, r2 = (vec(c) for _ in range(4))
    yw = wide(y, ldy)
    xo = gout((npix, ldo)); up = gout((B, 2 * h, 2 * w, ldu))
    ops.bn_apply_fused(None, 0, c, npix, gamma, beta, 1e-3, 0.99, False, mm, mv, s2, h2, m2, r2, yw, ldy, True, xo, ldo, up, ldu, h, w)
    torch.cuda.synchronize()
    ref, _ = O.batch_norm(y.float().reshape(1, 1, npix, c), gamma.cpu(), beta.cpu(), mm.cpu(), mv.cpu(), False)
    ref = torch.relu(ref).reshape(npix, c)
    close(xo[:, :c], ref, 1e-2, 2e-3, 'bn_apply_fused(up)/x_out')
    xc = dev(xo[:, :c].cpu().contiguous())
    up_r = gout((B, 2 * h, 2 * w, c))
    ops.upsample2x_fwd(xc.reshape(B, h, w, c), up_r, B, h, w, c, c, c)
    torch.cuda.synchronize()
    assert torch.equal(up[..., :c], up_r), 'the fused up-sampled output differs from imm_upsample2x_fwd of the stored tensor'
    close(up[..., :c], O.resize_bilinear(xo[:, :c].float().cpu().reshape(B, h, w, c), 2 * h, 2 * w), 8e-3, 1e-3, 'bn_apply_fused(up)/up')
    assert untouched(xo[:, c:]) and untouched(up[..., c:]), 'imm_bn_apply_fused wrote columns [c, ld) of an output'
    # x_out == NULL: only the up-sampled tensor
    up2 = gout((B, 2 * h, 2 * w, ldu))
    ops.bn_apply_fused(None, 0, c, npix, gamma, beta, 1e-3, 0.99, False, mm, mv, s2, h2, m2, r2, yw, ldy, True, None, 0, up2, ldu, h, w)
    torch.cuda.synchronize()
    assert torch.equal(up2[..., :c], up_r) and untouched(up2[..., c:])


# ----------------------------------------------------------------------------------------------
# align_corners resize       (A: the engine's (e.ldo, Cj) / (Cj, nf8) pairs;  B: non-square, unequal ratios)
# ----------------------------------------------------------------------------------------------
RESIZE_CASES = [
    # B, hi, wi, ho, wo, c, ld of the large tensor, ld of the small one
    (2, 8, 8, 4, 4, 256, 256, 288),          # engine forward (e.ldo = nf8, Cj) and backward (Cj, nf8) at S = 256
    (2, 8, 8, 4, 4, 256, 264, 320),
    (2, 32, 32, 16, 16, 16, 24, 32),         # the existing shape, wide on both sides
    (2, 32, 48, 16, 24, 16, 16, 16),
    (2, 48, 32, 24, 16, 16, 16, 24),
    (2, 32, 64, 16, 16, 16, 24, 16),         # ratio 31/15 down the rows, 63/15 along them
    (2, 64, 32, 16, 16, 16, 16, 16),
]


@pytest.mark.parametrize('B,hi,wi,ho,wo,c,ldx,ldy', RESIZE_CASES, ids=['b%d_%dx%d_to_%dx%d_c%d_ld%d_%d' % t for t in RESIZE_CASES])
def test_resize_align_corners_strides_and_non_square(ops, B, hi, wi, ho, wo, c, ldx, ldy):
    x = rnd((B, hi, wi, c), 53)
    xr = x.float().requires_grad_(True)
    ref = O.resize_bilinear(xr, ho, wo, align_corners=True)
    y = gout((B, ho, wo, ldy))
    ops.resize_ac_fwd(wide(x, ldx), y, B, hi, wi, ho, wo, c, ldx, ldy)
    dy = rnd((B, ho, wo, c), 54)
    (gx,) = torch.autograd.grad(ref, xr, dy.float())
    dx = gout((B, hi, wi, ldx))
    ops.resize_ac_bwd(wide(dy, ldy), dx, B, hi, wi, ho, wo, c, ldy, ldx)
    torch.cuda.synchronize()
    close(y[..., :c], ref, 8e-3, 2e-3, 'resize_ac_fwd')
    close(dx[..., :c], gx, 8e-3, 2e-3, 'resize_ac_bwd')
    assert untouched(y[..., c:]) and untouched(dx[..., c:]), 'imm_resize_ac_fwd / _bwd wrote columns [c, ld) of an output'


# ----------------------------------------------------------------------------------------------
# max pool (no stride parameter)        (B: (8, 12) and (12, 8))
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', [(8, 12), (12, 8)])
def test_maxpool_non_square(ops, h, w):
    B, c = 3, 16
    x = torch.relu(rnd((B, h, w, c), 55))
    xr = x.float().requires_grad_(True)
    ref = O.max_pool2(xr)
    y = gout((B, h // 2, w // 2, c))
    xd = dev(x)
    ops.maxpool2_fwd(xd, y, B, h, w, c)
    torch.cuda.synchronize()
    assert torch.equal(y.float().cpu(), ref.detach())
    dy = rnd((B, h // 2, w // 2, c), 56)
    (gx,) = torch.autograd.grad(ref, xr, dy.float())
    for relu_mask in (0, 1):
        dx = gout((B, h, w, c))
        ops.maxpool2_bwd(xd, dev(dy), dx, B, h, w, c, relu_mask)
        torch.cuda.synchronize()
        if relu_mask:
            assert torch.equal(dx.float().cpu(), gx * (x.float() > 0))
        else:
            assert torch.equal((dx.float().cpu() * (x.float() > 0)), gx * (x.float() > 0))
            np.testing.assert_allclose(float(dx.float().sum()), float(dy.float().sum()), rtol=1e-3)


# ----------------------------------------------------------------------------------------------
# bias gradient       (A: ld > c > c_out)
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('npix,c,c_out,ld', [(1000, 16, 10, 24), (3000, 16, 10, 32), (1000, 32, 30, 64)])
def test_colsum_strides(ops, npix, c, c_out, ld):
    dy = rnd((npix, c_out), 31)
    row = torch.zeros(npix, c, dtype=dy.dtype)
    row[:, :c_out] = dy                                  # [c_out, c): the zero padding of a convolution's output gradient
    dd = wide(row, ld)
    part = gout((ops.colsum_blocks(npix, c), c), torch.float32)
    out = vec(c)
    ops.colsum(dd, npix, c, c_out, ld, part, out)
    torch.cuda.synchronize()
    close(out[:c_out], dy.float().sum(0), 1e-4, 1e-5, 'colsum')
    assert untouched(out[c_out:]), 'imm_colsum wrote entries >= c_out'


# ----------------------------------------------------------------------------------------------
# image-space loss gradient         (A: ldp, lddp; new kernel test)
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('l1', [False, True], ids=['squared', 'l1'])
@pytest.mark.parametrize('ldp,lddp', [(3, 8), (8, 16), (12, 8), (12, 16)])
def test_image_loss_grad(ops, ldp, lddp, l1, dt):
    """imm_image_loss_grad — the backward of reconstruction_loss 'l2' (imm_model.py:385-387): dpred[p][ch] = coef[idx] * mask[p] *
    (pred - gt) for ch < 3 (sign(.) with l1), ZERO for the other lddp - 3 channels of the gradient image, which the kernel owns.
    Against autograd of the oracle's loss expression (oracle.forward: 1000 * mean(mask * (pred - gt)^2) / 255) with a random mask
    that differs from sample to sample (synthetic_inputs repeats one mask over the batch: a wrong batch index is invisible at step
    level); coef[idx] is what imm_perceptual_finalize(IMM_LOSS_L2) writes, (1000 / 255) * 2 / nel, at idx = 2 of a table whose
    other entries would show.  One rounding of the 16-bit store: 2^-8 bf16, 2^-11 f16 (the tolerances of test_conv_forward)."""
    B, S = 3, 20                                        # 1200 pixels: ragged against the 256-thread blocks
    g = torch.Generator().manual_seed(7 + ldp + lddp)
    gt = torch.rand(B, S, S, 3, generator=g) * 255
    pred = torch.rand(B, S, S, 3, generator=g) * 255
    mask = torch.rand(B, S, S, generator=g)
    assert not torch.equal(mask[0], mask[1])
    nel = float(B * S * S * 3)
    ck = (1000.0 / 255.0) * 2.0 / nel
    pr = pred.clone().requires_grad_(True)
    if l1:
        loss = ck * (mask.unsqueeze(-1) * (pr - gt).abs()).sum()
    else:
        loss = 1000.0 * ((pr - gt) ** 2 * mask.unsqueeze(-1)).mean() / 255.0
    (gp,) = torch.autograd.grad(loss, pr)
    coef = dev(torch.tensor([123.0, -7.0, ck, 55.0]))
    predw, gtd, maskd = wide(pred, ldp), dev(gt), dev(mask)
    rt = 1e-2 if dt == torch.bfloat16 else 2e-3
    dpred = gout((B, S, S, lddp), dt)
    ops.image_loss_grad(gtd, predw, ldp, B, S, maskd, coef, 2, dpred, lddp, l1)
    torch.cuda.synchronize()
    close(dpred[..., :3], gp, rt, 2e-3, 'image_loss_grad')
    assert float(dpred[..., 3:].float().abs().max()) == 0.0, 'channels [3, lddp) of the gradient image are written as zeros'
    # no mask (loss_mask: False): mask == 1
    pr2 = pred.clone().requires_grad_(True)
    loss2 = ck * (pr2 - gt).abs().sum() if l1 else 1000.0 * ((pr2 - gt) ** 2).mean() / 255.0
    (gp2,) = torch.autograd.grad(loss2, pr2)
    dpred2 = gout((B, S, S, lddp), dt)
    ops.image_loss_grad(gtd, predw, ldp, B, S, None, coef, 2, dpred2, lddp, l1)
    torch.cuda.synchronize()
    close(dpred2[..., :3], gp2, rt, 2e-3, 'image_loss_grad (no mask)')
    assert float(dpred2[..., 3:].float().abs().max()) == 0.0


def test_image_loss_grad_rejects_unserved_strides(ops):
    from imm_amd import _lib as L
    z = gout((1, 4, 4, 3), torch.float32, fill=0)
    coef = vec(1, 0)
    with pytest.raises(L.ImmHipError, match='image_loss_grad: lddp=12 must be a multiple of 8'):
        ops.image_loss_grad(z, z, 3, 1, 4, None, coef, 0, gout((1, 4, 4, 12)), 12)
    with pytest.raises(L.ImmHipError, match='image_loss_grad: args'):
        ops.image_loss_grad(z, z, 2, 1, 4, None, coef, 0, gout((1, 4, 4, 8)), 8)


@pytest.mark.parametrize('ldp,lddp', [(3, 8), (8, 16), (12, 8)])
def test_vgg_conv1_1_bwd_strides(ops, ldp, lddp):
    """imm_vgg_conv1_1_bwd with ldp != lddp (test_vgg_conv1_1: both 16) and a per-sample different mask."""
    B, S = 2, 32
    g = torch.Generator().manual_seed(70 + ldp)
    gt = torch.rand(B, S, S, 3, generator=g) * 255
    pred = torch.rand(B, S, S, 3, generator=g) * 255
    w = rnd((3, 3, 1, 64), 71, 0.4, torch.float32); b = rnd((64,), 72, 0.1, torch.float32)
    pr = pred.clone().requires_grad_(True)
    gray = pr.mean(dim=3, keepdim=True) / 255.0 - O.VGG_GRAY_MEAN / 255.0
    ref = torch.relu(O.conv2d_same(gray, w, b))
    dz = rnd((B, S, S, 64), 73) * (ref.detach() > 0)
    mask = torch.rand(B, S, S, generator=g)
    coef = torch.tensor([9.0, 0.37, 0, 0, 0, 0])
    loss = (ref * dz.float()).sum() + 0.5 * 0.37 * (mask.unsqueeze(-1) * (pr - gt) ** 2).sum()
    (gp,) = torch.autograd.grad(loss, pr)
    dpred = gout((B, S, S, lddp))
    ops.vgg_conv1_1_bwd(dev(dz), B, S, dev(w.reshape(9, 64).contiguous()), dev(gt), wide(pred, ldp), ldp, dev(mask), dev(coef), dpred, lddp,
                        input_idx=1)
    torch.cuda.synchronize()
    close(dpred[..., :3], gp, 1e-2, 2e-3, 'vgg1_1_bwd')
    assert float(dpred[..., 3:].float().abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------
# landmark bottleneck          (A: ldf > C, lddf > C;  B: (16, 32) and (32, 16), K in {10, 30})
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['rot', 'flat', 'ankush'])
@pytest.mark.parametrize('h,w,K', [(16, 32, 10), (32, 16, 10), (16, 32, 30), (32, 16, 30)])
def test_softargmax_gauss_non_square(ops, h, w, K, mode):
    """test_softargmax_gauss on h != w heat-maps: py is [B, h, K], px is [B, w, K]; the heat-map rows carry NaN in [K, ldh)."""
    B, s, ldh, ldg = 3, 16, ops.round_up(K, 4) + 4, ops.round_up(256 + K, 32)
    heat = rnd((B, h, w, K), 61, 2.0, torch.float32)
    hr = heat.clone().requires_grad_(True)
    mu_r, py_r, px_r = O.soft_argmax(hr)
    g_r = O.gaussian_maps(mu_r, [s, s], 10.0, mode)
    mu = gout((B, K, 2), torch.float32); py = gout((B, h, K), torch.float32); px = gout((B, w, K), torch.float32)
    joint = gout((B, s, s, ldg))
    ops.softargmax_gauss_fwd(wide(heat, ldh), ldh, B, h, w, K, 10.0, s, mu, py, px, joint[..., 256:], ldg, torch.bfloat16, mode)
    torch.cuda.synchronize()
    close(mu, mu_r, 1e-4, 1e-5, 'mu')
    assert float((mu.cpu() - mu_r.detach()).abs().max()) < 1e-5
    close(py, py_r, 1e-4, 1e-5, 'py'); close(px, px_r, 1e-4, 1e-5, 'px')
    close(joint[..., 256:256 + K], g_r, 8e-3, 1e-3, 'gauss')
    assert untouched(joint[..., :256]) and untouched(joint[..., 256 + K:]), 'the maps own columns [256, 256 + K) of the concat buffer'
    dg = rnd((B, s, s, K), 62)
    (gh,) = torch.autograd.grad(g_r, hr, dg.float())
    dj = torch.full((B, s, s, ldg), NAN, dtype=torch.bfloat16)
    dj[..., 256:256 + K] = dg
    dj = dev(dj)
    dheat = gout((B, h, w, 64))
    ops.softargmax_gauss_bwd(dj[..., 256:], ldg, B, h, w, K, 10.0, s, mu, py, px, dheat, 64, mode)
    torch.cuda.synchronize()
    close(dheat[..., :K], gh, 1e-2, 2e-3, 'dheat')
    assert float(dheat[..., K:].float().abs().max()) == 0.0


POSE_CASES = [
    # h, w, K, mode, ldf, lddf
    (16, 16, 10, 'rot', 264, 288),           # A: the existing shape, feature rows wider than C on both sides
    (16, 16, 10, 'ankush', 288, 264),
    (16, 32, 10, 'rot', 256, 256),           # B
    (32, 16, 10, 'rot', 264, 256),
    (16, 32, 30, 'rot', 256, 264),
    (32, 16, 30, 'rot', 256, 256),
]


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('h,w,K,mode,ldf,lddf', POSE_CASES, ids=['%dx%d_k%d_%s_ldf%d_lddf%d' % t for t in POSE_CASES])
def test_pose_head_strides_and_non_square(ops, h, w, K, mode, ldf, lddf, dt):
    """imm_pose_head_fwd / _bwd against the oracle as in test_pose_head_fused (1x1 convolution + soft-argmax + Gaussian maps,
    autograd for the backward), with ldf > C, lddf > C and h != w."""
    B, C, s = 3, 256, 16
    ldh, ldg, lddh = ops.round_up(K, 4), ops.round_up(C + K, 64), ops.round_up(K, 32)
    feat = rnd((B, h, w, C), 161, 1.0, dt)
    wgt = rnd((1, 1, C, K), 162, 0.05, dt)
    bias = rnd((K,), 163, 0.3, torch.float32)
    fr = feat.float().clone().requires_grad_(True)
    wr = wgt.float().clone().requires_grad_(True)
    br = bias.clone().requires_grad_(True)
    heat_r = O.conv2d_same(fr, wr, br, 1)
    mu_r, py_r, px_r = O.soft_argmax(heat_r)
    g_r = O.gaussian_maps(mu_r, [s, s], 10.0, mode)
    fd = ops.fwd_desc(B, h, w, C, ldf, K, ldh, 1, 1, 0)
    wt = gout((128, fd.kpad), dt, fill=0)
    wd = dev(wgt.float().contiguous())
    ops.pack_weights(wd, wt, 0, 1, 1, C, K, C, 128, fd.kpad)
    heat = gout((B, h, w, ldh), torch.float32)
    mu = gout((B, K, 2), torch.float32); py = gout((B, h, K), torch.float32); px = gout((B, w, K), torch.float32)
    joint = gout((B, s, s, ldg), dt)
    ops.pose_head_fwd(wide(feat, ldf), ldf, C, wt, dev(bias), B, h, w, K, 10.0, s, heat, ldh, mu, py, px, joint[..., C:], ldg, dt, mode)
    torch.cuda.synchronize()
    close(heat[..., :K], heat_r, 2e-3, 2e-4, 'heat')
    assert untouched(heat[..., K:]), 'imm_pose_head_fwd wrote columns [K, ldh) of the heat-map'
    assert float((mu.cpu() - mu_r.detach()).abs().max()) < 2e-5
    close(py, py_r, 1e-3, 1e-5, 'py'); close(px, px_r, 1e-3, 1e-5, 'px')
    close(joint[..., C:C + K], g_r, 8e-3 if dt == torch.bfloat16 else 2e-3, 1e-3, 'gauss')
    assert untouched(joint[..., :C]) and untouched(joint[..., C + K:]), 'the maps own columns [C, C + K) of the concat buffer'
    # ---- backward
    dg = rnd((B, s, s, K), 164, 1.0, dt)
    gf, gw, gb = torch.autograd.grad(g_r, (fr, wr, br), dg.float())
    dj = torch.full((B, s, s, ldg), NAN, dtype=dt)
    dj[..., C:C + K] = dg
    dj = dev(dj)
    wtd = gout((ops.round_up(C, 128), lddh), dt, fill=0)
    ops.pack_weights(wd, wtd, 1, 1, 1, C, K, lddh, wtd.shape[0], lddh)
    dheat = gout((B, h, w, lddh), dt)
    dfeat = gout((B, h, w, lddf), dt)
    bpart = gout((B, K), torch.float32)
    ops.pose_head_bwd(dj[..., C:], ldg, B, h, w, K, 10.0, s, mu, py, px, dheat, lddh, wtd, C, dfeat, lddf, bpart, mode)
    dheat2 = gout(dheat.shape, dt)
    ops.softargmax_gauss_bwd(dj[..., C:], ldg, B, h, w, K, 10.0, s, mu, py, px, dheat2, lddh, mode)
    torch.cuda.synchronize()
    assert torch.equal(dheat, dheat2)
    assert float(dheat[..., K:].float().abs().max()) == 0.0
    tol = 1e-2 if dt == torch.bfloat16 else 2e-3
    close(dfeat[..., :C], gf, tol, 2e-3, 'dfeat')
    assert untouched(dfeat[..., C:]), 'imm_pose_head_bwd wrote columns [C, lddf) of dfeat'
    # the per-sample column sums of the STORED dheat, against their f64 sum (an f32 sum of these 3 h w cancelling terms in another
    # order differs from the kernel's by as much as the bound itself)
    got_b, want_b = bpart.double().sum(0).cpu(), dheat[..., :K].double().sum((0, 1, 2)).cpu()
    print('POSE_BIAS %dx%d k%d %s: max|bias_partial - sum dheat| %.3g, max sum|dheat| %.3g' % (
        h, w, K, str(dt)[6:], float((got_b - want_b).abs().max()), float(dheat[..., :K].double().abs().sum((0, 1, 2)).max())))
    np.testing.assert_allclose(got_b.numpy(), want_b.numpy(), rtol=1e-5, atol=1e-6)
    close(torch.einsum('bhwc,bhwk->ck', feat.float(), dheat[..., :K].float().cpu()).reshape(1, 1, C, K), gw, tol, 5e-3, 'dW from dheat')


# ----------------------------------------------------------------------------------------------
# tap-unrolled first-layer input          (B: one tall, one wide; ld above 3 * kw)
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,ld', [(12, 20, 32), (20, 12, 40), (9, 7, 24)])
def test_pack_image_taps_non_square(ops, h, w, ld):
    """dst[b, y, x, kx * 3 + ch] = src[b, y, x + kx - 3, ch], zero outside the image; the kernel owns the whole row: [21, ld) = 0."""
    B = 2
    src = torch.rand(B, h, w, 3, generator=torch.Generator().manual_seed(h)) * 255
    xin = gout((B, h, w, ld))
    ops.pack_image_taps(dev(src), xin, B, h, w, 7, 3, ld)
    torch.cuda.synchronize()
    xp = torch.nn.functional.pad(src.to(torch.bfloat16), (0, 0, 3, 3))
    for kx in range(7):
        assert torch.equal(xin[..., kx * 3:kx * 3 + 3].cpu(), xp[:, :, kx:kx + w]), kx
    assert float(xin[..., 21:].float().abs().max()) == 0.0
