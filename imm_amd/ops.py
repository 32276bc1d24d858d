"""Thin torch-tensor -> C-ABI wrappers.  Every function launches on torch's CURRENT stream and returns
immediately; tensors are caller-allocated device buffers (PyTorch is only the allocator here).
"""
import ctypes as C

import torch

from . import _lib as L
from ._lib import ConvDesc, OptHParams, call  # noqa: F401


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def dtype_enum(dt):
    if dt == torch.bfloat16:
        return L.IMM_BF16
    if dt == torch.float16:
        return L.IMM_F16
    if dt == torch.float32:
        return L.IMM_F32          # the f32 witness engine (plain f32 kernels; imm_amd/csrc/conv_f32.hip)
    raise ValueError('activation dtype must be torch.bfloat16 / torch.float16 (or torch.float32: the witness engine), got %r' % (dt,))


def round_up(x, m):
    return (x + m - 1) // m * m


def same_pad_before(n_in, k, s):
    """TF SAME: pad_before = max((ceil(in/s)-1)*s + k - in, 0) // 2  (SURVEY.md §8a S1)."""
    n_out = -(-n_in // s)
    return max((n_out - 1) * s + k - n_in, 0) // 2, n_out


def fwd_desc(batch, hi, wi, ci, ldx, co, ldy, k, stride, flags, ldmask=0, kw=None):
    """k x k SAME convolution; kw (e.g. 1) gives a k x kw kernel (SAME along both axes)."""
    kw = k if kw is None else kw
    pt, ho = same_pad_before(hi, k, stride)
    pl, wo = same_pad_before(wi, kw, stride)
    return ConvDesc(batch=batch, hi=hi, wi=wi, ci=ci, ldx=ldx, ho=ho, wo=wo, co=co, ldy=ldy, kh=k, kw=kw,
                    stride=stride, pad_t=pt, pad_l=pl, updiv=1, kpad=round_up(k * kw * ci, 32), flags=flags,
                    ldmask=ldmask)


def dgrad_desc(batch, hi, wi, ci_out, lddx, co_pad, lddy, k, stride, flags, ldmask=0):
    """Data gradient of the forward conv (hi,wi,ci)->(ho,wo,co): a conv of dy [ho,wo,co_pad] producing
    dx [hi,wi,ci_out] with flipped weights, stride 1, updiv = forward stride, pad = k-1-pad_fwd."""
    pt, ho = same_pad_before(hi, k, stride)
    pl, wo = same_pad_before(wi, k, stride)
    return ConvDesc(batch=batch, hi=ho, wi=wo, ci=co_pad, ldx=lddy, ho=hi, wo=wi, co=ci_out, ldy=lddx, kh=k, kw=k,
                    stride=1, pad_t=k - 1 - pt, pad_l=k - 1 - pl, updiv=stride, kpad=round_up(k * k * co_pad, 32),
                    flags=flags, ldmask=ldmask)


def dgrad_s2_class_descs(batch, hi, wi, ci_out, lddx, co_pad, lddy, k, flags=0, ldmask=0):
    """Stride-2 data gradient as 4 dense stride-1 convolutions, one per input-pixel parity class (py,px):
        dx[2a+py][2b+px] = sum_{ty,tx} dy[a-ty][b-tx] * W[py+2ty][px+2tx]
    (TF SAME on an even side with k=3 pads 0 before, so ky = iy - 2*oy has the parity of iy).  Returns
    [(desc, pack_mode)], or None when the geometry does not fit (odd side / pad_before != 0)."""
    pt, ho = same_pad_before(hi, k, 2)
    pl, wo = same_pad_before(wi, k, 2)
    if pt != 0 or pl != 0 or hi != 2 * ho or wi != 2 * wo:
        return None
    out = []
    for py in (0, 1):
        for px in (0, 1):
            ny, nx = (k - py + 1) // 2, (k - px + 1) // 2
            d = ConvDesc(batch=batch, hi=ho, wi=wo, ci=co_pad, ldx=lddy, ho=ho, wo=wo, co=ci_out, ldy=lddx, kh=ny, kw=nx,
                         stride=1, pad_t=ny - 1, pad_l=nx - 1, updiv=1, kpad=round_up(ny * nx * co_pad, 32), flags=flags,
                         ldmask=ldmask, out_scale=2, out_off_y=py, out_off_x=px)
            out.append((d, 4 + 2 * py + px))
    return out


def device_info():
    out = (C.c_int32 * 2)()
    call('imm_device_info', C.cast(out, C.c_void_p))
    return int(out[0]), int(out[1])


# ---- graph capture ---------------------------------------------------------------------------
class Graph:
    """A captured launch sequence (HIP graph) on torch's current stream."""

    def __init__(self):
        self._exec = C.c_void_p()

    def capture_begin(self):
        call('imm_graph_begin', _s())

    def capture_end(self):
        call('imm_graph_end', _s(), C.byref(self._exec))

    def launch(self):
        call('imm_graph_launch', self._exec, _s())

    def __del__(self):
        try:
            if self._exec:
                L.load().imm_graph_destroy(self._exec)
        except Exception:
            pass


# ---- weights / conv --------------------------------------------------------------------------
def pack_weights(w, wt, mode, kh, kw, ci_real, co_real, c_pad, rows, kpad):
    call('imm_pack_weights', _p(w), _p(wt), dtype_enum(wt.dtype), mode, kh, kw, ci_real, co_real, c_pad, rows, kpad, _s())


class JobTable:
    """Device job table for the table-driven launches (imm_pack_weights_multi / imm_wgrad_reduce_multi)."""

    def __init__(self, jobs, items_per_job, items_per_block, device, blocks_per_job=None):
        first = [0]
        if blocks_per_job is None:
            blocks_per_job = [max(1, -(-int(n) // items_per_block)) for n in items_per_job]
        for n in blocks_per_job:
            first.append(first[-1] + int(n))
        rows = [list(j) + [0] * (12 - len(j)) for j in jobs]
        self.jobs = torch.tensor(rows, dtype=torch.int64, device=device)
        self.blk_first = torch.tensor(first, dtype=torch.int32, device=device)
        self.n_jobs, self.n_blocks = len(jobs), first[-1]


def pack_table(jobs, device):
    """Job table of imm_pack_weights_multi: jobs = (w, wt, mode, kh, kw, ci_real, co_real, c_pad, rows, kpad) tuples."""
    blocks = []
    for j in jobs:
        n = L.load().imm_pack_weights_multi_blocks(int(j[2]), int(j[8]), int(j[9]))
        if n <= 0:
            raise L.ImmHipError('imm_pack_weights_multi_blocks(%d, %d, %d) failed' % (j[2], j[8], j[9]))
        blocks.append(n)
    return JobTable(jobs, None, None, device, blocks_per_job=blocks)


def pack_weights_multi(tab, dtype):
    call('imm_pack_weights_multi', _p(tab.jobs), _p(tab.blk_first), tab.n_jobs, tab.n_blocks, dtype_enum(dtype), _s())


def reduce_table(jobs, outputs_per_job, device):
    """Job table of imm_wgrad_reduce_multi: jobs = (slab, dw, nsplit, taps, ci_pad, ci_real, co, kpad) tuples; the split-lane
    count of a job (field 8) is the power of two next to its slab count, capped at 16."""
    rows, blocks = [], []
    for j, n in zip(jobs, outputs_per_job):
        lanes = 1
        while lanes < min(16, int(j[2])):
            lanes *= 2
        rows.append(tuple(j[:8]) + (lanes,))
        blocks.append(max(1, -(-int(n) // (1024 // lanes))))
    return JobTable(rows, None, None, device, blocks_per_job=blocks)


def wgrad_reduce_multi(tab):
    call('imm_wgrad_reduce_multi', _p(tab.jobs), _p(tab.blk_first), tab.n_jobs, tab.n_blocks, _s())


def conv2d(desc, x, wt, bias, y, stats=None, mask=None):
    call('imm_conv2d', C.byref(desc), dtype_enum(x.dtype), _p(x), _p(wt), _p(bias), _p(y), _p(stats), _p(mask), _s())


def conv2d_tap_supported(desc):
    return bool(L.load().imm_conv2d_tap_supported(C.byref(desc)))


def conv2d_tap(desc, x, wt, y, a_pred, a_gt, lda, loss_mask, S, coef, idx, l1=False):
    call('imm_conv2d_tap', C.byref(desc), dtype_enum(x.dtype), _p(x), _p(wt), _p(y), _p(a_pred), _p(a_gt), lda, _p(loss_mask), S,
         _p(coef), idx, int(l1), _s())


def conv_stats_blocks(desc):
    n = L.load().imm_conv_stats_blocks(C.byref(desc))
    if n <= 0:
        raise L.ImmHipError('imm_conv_stats_blocks: ' + L.load().imm_last_error().decode())
    return n


def conv2d_wgrad(desc, x, dy, lddy, slab, nsplit):
    call('imm_conv2d_wgrad', C.byref(desc), dtype_enum(x.dtype), _p(x), _p(dy), lddy, _p(slab), nsplit, _s())


CONV_FAMILIES = {1: 'igemm', 2: 'igemm64', 3: 'halo', 4: 'halo2', 5: 'hdeep', 6: 'hdeep6', 7: 's2f', 8: 'f32'}


def conv2d_variant(desc, dtype):
    """(family name, variant key) of the kernel imm_conv2d dispatches `desc` to (imm_conv2d_variant: family * 100000 + tile
    variant; families in CONV_FAMILIES) — what a test asserts to prove that the kernel a case is named after is the one that ran."""
    key = L.load().imm_conv2d_variant(C.byref(desc), dtype_enum(dtype))
    if key < 0:
        raise L.ImmHipError('imm_conv2d_variant: ' + L.load().imm_last_error().decode())
    return CONV_FAMILIES[key // 100000], key


def conv2d_wgrad_variant(desc, lddy, dtype):
    """(variant key, workgroups per pixel split, length in units, resident workgroups per CU) of a layer's filter-gradient
    kernel: jobs with the same key share a launch of imm_conv2d_wgrad_multi."""
    wps, units, pcu = C.c_int(0), C.c_int(0), C.c_int(0)
    key = L.load().imm_conv2d_wgrad_variant(C.byref(desc), lddy, dtype_enum(dtype), C.byref(wps), C.byref(units), C.byref(pcu))
    if key < 0:
        raise L.ImmHipError('imm_conv2d_wgrad_variant: ' + L.load().imm_last_error().decode())
    return key, wps.value, units.value, pcu.value


class WgradMulti(object):
    """Planned multi-problem filter-gradient launch: jobs = [(desc, x, dy, lddy, slab, nsplit[, (x_scale, x_shift, x_relu)])];
    the optional triple = normalise on load (x is the raw output of the conv + BN + ReLU block in front of the layer).  Keeps
    the host table, its device copy and the operand tensors alive."""

    def __init__(self, jobs, dtype):
        n = len(jobs)
        self.keep = [t for j in jobs for t in (j[1], j[2], j[4])] + [t for j in jobs if len(j) > 6 and j[6] for t in j[6][:2]]
        arr = (L.WgradJob * n)()
        for i, job in enumerate(jobs):
            desc, x, dy, lddy, slab, nsplit = job[:6]
            arr[i].desc = desc
            arr[i].x, arr[i].dy, arr[i].slab = x.data_ptr(), dy.data_ptr(), slab.data_ptr()
            arr[i].lddy, arr[i].nsplit = int(lddy), int(nsplit)
            if len(job) > 6 and job[6]:
                arr[i].x_scale, arr[i].x_shift, arr[i].x_relu = job[6][0].data_ptr(), job[6][1].data_ptr(), int(bool(job[6][2]))
        nbytes = L.load().imm_conv2d_wgrad_multi_table_bytes(n)
        if nbytes <= 0:
            raise L.ImmHipError('imm_conv2d_wgrad_multi_table_bytes(%d)' % n)
        self.host = (C.c_ubyte * nbytes)()
        call('imm_conv2d_wgrad_multi_plan', C.cast(arr, C.c_void_p), n, dtype_enum(dtype), C.cast(self.host, C.c_void_p))
        self.dev = torch.frombuffer(self.host, dtype=torch.uint8).clone().to(jobs[0][1].device)
        self.n = n


def conv2d_wgrad_multi(multi):
    call('imm_conv2d_wgrad_multi', C.cast(multi.host, C.c_void_p), _p(multi.dev), _s())


def conv2d_wgrad_splits(desc, lddy):
    n = L.load().imm_conv2d_wgrad_splits(C.byref(desc), lddy)
    if n < 0:
        raise L.ImmHipError('imm_conv2d_wgrad_splits failed')
    return n


def conv2d_wgrad_reduce(slab, nsplit, kh, kw, ci_pad, ci_real, co, kpad, dw):
    call('imm_conv2d_wgrad_reduce', _p(slab), nsplit, kh, kw, ci_pad, ci_real, co, kpad, _p(dw), _s())


def colsum_blocks(npix, c):
    n = L.load().imm_colsum_blocks(npix, c)
    if n <= 0:
        raise L.ImmHipError('imm_colsum_blocks(%d,%d) unsupported' % (npix, c))
    return n


def colsum(dy, npix, c, c_out, ld, partial, out):
    call('imm_colsum', _p(dy), dtype_enum(dy.dtype), npix, c, c_out, ld, _p(partial), _p(out), _s())


# ---- batch norm ------------------------------------------------------------------------------
def bn_finalize(partial, nblk, c, count, gamma, beta, eps, momentum, training, mm, mv, scale, shift, mean, rstd):
    call('imm_bn_finalize', _p(partial), nblk, c, count, _p(gamma), _p(beta), eps, momentum, int(training), _p(mm),
         _p(mv), _p(scale), _p(shift), _p(mean), _p(rstd), _s())


def bn_apply_relu(y, npix, c, ldy, scale, shift, relu, x_out, ldx):
    call('imm_bn_apply_relu', _p(y), dtype_enum(y.dtype), npix, c, ldy, _p(scale), _p(shift), int(relu), _p(x_out), ldx, _s())


def bn_apply_fused(partial, nblk, c, count, gamma, beta, eps, momentum, training, mm, mv, scale, shift, mean, rstd, y, ldy,
                   relu, x_out, ldx, up2x=None, ldu=0, h=0, w=0):
    call('imm_bn_apply_fused', _p(partial), nblk, c, count, _p(gamma), _p(beta), eps, momentum, int(training), _p(mm), _p(mv),
         _p(scale), _p(shift), _p(mean), _p(rstd), _p(y), dtype_enum(y.dtype), ldy, int(relu), _p(x_out), ldx,
         _p(up2x), ldu, h, w, _s())


def bn_bwd_apply_fused(partial, nblk, c, count, gamma, dout, lddo, y, ldy, scale, shift, mean, rstd, relu, dgamma, dbeta,
                       dy_out, lddy):
    call('imm_bn_bwd_apply_fused', _p(partial), nblk, c, count, _p(gamma), _p(dout), lddo, _p(y), ldy, dtype_enum(y.dtype),
         _p(scale), _p(shift), _p(mean), _p(rstd), int(relu), _p(dgamma), _p(dbeta), _p(dy_out), lddy, _s())


def bn_bwd_blocks(npix, c):
    n = L.load().imm_bn_bwd_blocks(npix, c)
    if n <= 0:
        raise L.ImmHipError('imm_bn_bwd_blocks(%d,%d) unsupported' % (npix, c))
    return n


def rows_reduce(src, rows, width, group, dst):
    """dst[g] = sum of rows [g*group, (g+1)*group) of src[rows][width] (include/imm_hip.h: imm_rows_reduce)."""
    call('imm_rows_reduce', _p(src), rows, width, group, _p(dst), _s())


def bn_bwd_reduce(dout, lddo, y, ldy, npix, c, scale, shift, mean, rstd, relu, partial):
    call('imm_bn_bwd_reduce', _p(dout), lddo, _p(y), ldy, dtype_enum(y.dtype), npix, c, _p(scale), _p(shift), _p(mean),
         _p(rstd), int(relu), _p(partial), _s())


def bn_bwd_reduce_up(dy_up, lddy, dprev, lddp, y, ldy, batch, h, w, c, scale, shift, mean, rstd, relu, partial):
    call('imm_bn_bwd_reduce_up', _p(dy_up), lddy, _p(dprev), lddp, _p(y), ldy, dtype_enum(y.dtype), batch, h, w, c, _p(scale),
         _p(shift), _p(mean), _p(rstd), int(relu), _p(partial), _s())


def bn_bwd_finalize(partial, nblk, c, count, gamma, beta, rstd, dgamma, dbeta, coef, from_out=False, ldp=None):
    call('imm_bn_bwd_finalize', _p(partial), nblk, c, c if ldp is None else ldp, count, _p(gamma), _p(beta), _p(rstd),
         int(from_out), _p(dgamma), _p(dbeta), _p(coef), _s())


def bn_bwd_apply(dout, lddo, y, ldy, npix, c, scale, shift, mean, rstd, relu, coef, dy_out, lddy):
    call('imm_bn_bwd_apply', _p(dout), lddo, _p(y), ldy, dtype_enum(y.dtype), npix, c, _p(scale), _p(shift), _p(mean),
         _p(rstd), int(relu), _p(coef), _p(dy_out), lddy, _s())


# ---- resampling / pooling ---------------------------------------------------------------------
def upsample2x_fwd(x, y, batch, h, w, c, ldx, ldy):
    call('imm_upsample2x_fwd', _p(x), _p(y), dtype_enum(x.dtype), batch, h, w, c, ldx, ldy, _s())


def upsample2x_bwd(dy, dx, batch, h, w, c, lddy, lddx):
    call('imm_upsample2x_bwd', _p(dy), _p(dx), dtype_enum(dy.dtype), batch, h, w, c, lddy, lddx, _s())


def upsample2x_bwd_bn_blocks(batch, h, w, c):
    n = L.load().imm_upsample2x_bwd_bn_blocks(batch, h, w, c)
    if n <= 0:
        raise L.ImmHipError('imm_upsample2x_bwd_bn_blocks(%d,%d,%d,%d) unsupported' % (batch, h, w, c))
    return n


def upsample2x_bwd_bn(dy, dx, batch, h, w, c, lddy, lddx, out, ldo, partial):
    call('imm_upsample2x_bwd_bn', _p(dy), _p(dx), dtype_enum(dy.dtype), batch, h, w, c, lddy, lddx, _p(out), ldo, _p(partial), _s())


def resize_ac_fwd(x, y, batch, hi, wi, ho, wo, c, ldx, ldy):
    call('imm_resize_ac_fwd', _p(x), _p(y), dtype_enum(x.dtype), batch, hi, wi, ho, wo, c, ldx, ldy, _s())


def resize_ac_bwd(dy, dx, batch, hi, wi, ho, wo, c, lddy, lddx):
    call('imm_resize_ac_bwd', _p(dy), _p(dx), dtype_enum(dy.dtype), batch, hi, wi, ho, wo, c, lddy, lddx, _s())


def maxpool2_fwd(x, y, batch, h, w, c):
    call('imm_maxpool2_fwd', _p(x), _p(y), dtype_enum(x.dtype), batch, h, w, c, _s())


def maxpool2_bwd(x, dy, dx, batch, h, w, c, relu_mask):
    call('imm_maxpool2_bwd', _p(x), _p(dy), _p(dx), dtype_enum(x.dtype), batch, h, w, c, int(relu_mask), _s())


def pack_image_taps(src, dst, batch, h, w, kw, pad_l, ld):
    call('imm_pack_image_taps', _p(src), _p(dst), dtype_enum(dst.dtype), batch, h, w, kw, pad_l, ld, _s())


def pack_image(src, dst, npix):
    call('imm_pack_image', _p(src), _p(dst), dtype_enum(dst.dtype), npix, _s())


# ---- bottleneck ------------------------------------------------------------------------------
def gauss_mode_enum(mode):
    if mode not in L.GAUSS_MODES:
        raise ValueError('Unknown mode: ' + str(mode))       # imm_model.py:75
    return L.GAUSS_MODES[mode]


def softargmax_gauss_fwd(heat, ldh, batch, h, w, k, inv_std, s, mu, py, px, gauss_out, ldg, dtype, mode='rot'):
    call('imm_softargmax_gauss_fwd', _p(heat), ldh, batch, h, w, k, float(inv_std), s, _p(mu), _p(py), _p(px),
         _p(gauss_out), ldg, dtype_enum(dtype), gauss_mode_enum(mode), _s())


def gauss_render_fwd(mu, batch, k, inv_std, s, gauss_out, ldg, dtype, mode='rot'):
    """Render-only mode of imm_softargmax_gauss_fwd (heat NULL): the 16-bit Gaussian maps of the INPUT landmarks mu f32 [B, K, 2]
    at gauss_out[((b*s + y)*s + x)*ldg + k], k < K only (bit-identical to the soft-argmax / pose-head writers' maps)."""
    call('imm_softargmax_gauss_fwd', None, 0, batch, 0, 0, k, float(inv_std), s, _p(mu), None, None, _p(gauss_out), ldg,
         dtype_enum(dtype), gauss_mode_enum(mode), _s())


def softargmax_gauss_bwd(dgauss, ldg, batch, h, w, k, inv_std, s, mu, py, px, dheat, lddh, mode='rot'):
    call('imm_softargmax_gauss_bwd', _p(dgauss), ldg, dtype_enum(dheat.dtype), batch, h, w, k, float(inv_std), s, _p(mu),
         _p(py), _p(px), _p(dheat), lddh, gauss_mode_enum(mode), _s())


MAX_KEYPOINTS = 16            # annotated points of the pose head's keypoint epilogue


def keypoint_desc(w, b, geom, keypoints, image_size):
    """The keypoint epilogue's descriptor (include/imm_hip.h: imm_keypoint_desc): w f32 [2K, 2M], b f32 [2M], geom f32 [>= batch, 4]
    (y0, x0, sy, sx), keypoints f32 [>= batch, M, 2]; all contiguous device tensors.  M is keypoints.shape[1]."""
    m = int(keypoints.shape[1])
    if not 1 <= m <= MAX_KEYPOINTS:
        raise ValueError('the keypoint epilogue serves 1..%d annotated points, got %d' % (MAX_KEYPOINTS, m))
    if tuple(w.shape[1:]) != (2 * m,) or tuple(b.shape) != (2 * m,) or geom.shape[1:] != (4,) or keypoints.shape[2:] != (2,):
        raise ValueError('keypoint descriptor shapes: w %s, b %s, geom %s, keypoints %s' % (
            tuple(w.shape), tuple(b.shape), tuple(geom.shape), tuple(keypoints.shape)))
    for t in (w, b, geom, keypoints):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError('keypoint descriptor tensors must be contiguous float32')
    return L.KeypointDesc(w.data_ptr(), b.data_ptr(), geom.data_ptr(), keypoints.data_ptr(), m, int(image_size))


def pose_head_fwd(feat, ldf, c, wt, bias, batch, h, w, k, inv_std, s, heat, ldh, mu, py, px, gauss_out, ldg, dtype, mode='rot',
                  keypoints=None):
    """keypoints: None, or the epilogue's descriptor (keypoint_desc(...)): the regressed annotated points in source pixels."""
    if keypoints is not None:
        if int(keypoints.m) > MAX_KEYPOINTS or k > 64:
            raise ValueError('the keypoint epilogue serves M <= %d, K <= 64 (M=%d, K=%d)' % (MAX_KEYPOINTS, int(keypoints.m), k))
        keypoints = C.byref(keypoints)
    call('imm_pose_head_fwd', _p(feat), ldf, c, _p(wt), wt.shape[1], _p(bias), dtype_enum(dtype), batch, h, w, k, float(inv_std), s,
         _p(heat), ldh, _p(mu), _p(py), _p(px), _p(gauss_out), ldg, gauss_mode_enum(mode), keypoints, _s())


def pose_head_bwd(dgauss, ldg, batch, h, w, k, inv_std, s, mu, py, px, dheat, lddh, wt_dgrad, c, dfeat, lddf, bias_partial, mode='rot'):
    call('imm_pose_head_bwd', _p(dgauss), ldg, dtype_enum(dheat.dtype), batch, h, w, k, float(inv_std), s, _p(mu), _p(py), _p(px),
         _p(dheat), lddh, gauss_mode_enum(mode), _p(wt_dgrad), wt_dgrad.shape[1], c, _p(dfeat), lddf, _p(bias_partial), _s())


def gauss_render_f32(mu, batch, k, inv_std, s, out, mode='rot'):
    call('imm_gauss_render_f32', _p(mu), batch, k, float(inv_std), s, _p(out), gauss_mode_enum(mode), _s())


# ---- VGG head / loss --------------------------------------------------------------------------
def vgg_head_supported(batch, s, dtype):
    """conv1_1 + conv1_2 of the frozen VGG16 in one launch (vgg_head.hip) serves this shape / storage type."""
    if dtype not in (torch.bfloat16, torch.float16):
        return False
    return bool(L.load().imm_vgg_head_supported(batch, s, dtype_enum(dtype)))


def vgg_head_scratch_bytes(batch, s):
    return int(L.load().imm_vgg_head_scratch_bytes(batch, s))


def vgg_head_fwd(gt, pred, ldp, batch, s, w11, b11, wt12, b12, a11, store_from, y12, gray_scratch):
    """gt f32 [B,S,S,3], pred f32 [B,S,S,ldp] -> y12 16-bit [2B,S,S,64] = relu(conv1_2(relu(conv1_1(gray(concat([gt, pred])))))),
    a11[store_from:] = conv1_1's activation of those images (selfsup/vgg16.py:345-346, build_vgg16.py:22-26)."""
    call('imm_vgg_head_fwd', _p(gt), _p(pred), ldp, batch, s, _p(w11), _p(b11), _p(wt12), wt12.shape[1], _p(b12), _p(a11),
         store_from, _p(y12), _p(gray_scratch), dtype_enum(y12.dtype), _s())


def vgg_conv1_1_fwd(gt, pred, ldp, batch, s, w, b, out, halves=3):
    call('imm_vgg_conv1_1_fwd', _p(gt), _p(pred), ldp, batch, s, _p(w), _p(b), _p(out), dtype_enum(out.dtype), halves, _s())


def vgg_conv1_1_bwd(dz, batch, s, w, gt, pred, ldp, mask, coef, dpred, lddp, input_idx=0, l1=False):
    call('imm_vgg_conv1_1_bwd', _p(dz), dtype_enum(dz.dtype), batch, s, _p(w), _p(gt), _p(pred), ldp, _p(mask), _p(coef),
         int(input_idx), int(l1), _p(dpred), lddp, _s())


def image_loss_grad(gt, pred, ldp, batch, s, mask, coef, idx, dpred, lddp, l1=False):
    call('imm_image_loss_grad', _p(gt), _p(pred), ldp, batch, s, _p(mask), _p(coef), int(idx), int(l1), _p(dpred), lddp,
         dtype_enum(dpred.dtype), _s())


def masked_sse(a, b, batch, s, c, mask, S, partial, l1=False):
    call('imm_masked_sse', _p(a), _p(b), dtype_enum(a.dtype), batch, s, c, _p(mask), S, int(l1), _p(partial), _s())


class SseMulti:
    """Argument block of imm_masked_sse_multi: feats = [(a, b, s, c, partial_row)], built once, launched every step."""

    def __init__(self, feats):
        n = len(feats)
        self.n = n
        self.keep = feats
        self.a = (C.c_void_p * n)(*[f[0].data_ptr() for f in feats])
        self.b = (C.c_void_p * n)(*[f[1].data_ptr() for f in feats])
        self.s = (C.c_int32 * n)(*[int(f[2]) for f in feats])
        self.c = (C.c_int32 * n)(*[int(f[3]) for f in feats])
        self.p = (C.c_void_p * n)(*[f[4].data_ptr() for f in feats])
        self.dtype = feats[0][0].dtype


def masked_sse_multi(g, batch, mask, S, l1=False):
    call('imm_masked_sse_multi', g.n, C.cast(g.a, C.c_void_p), C.cast(g.b, C.c_void_p), C.cast(g.s, C.c_void_p), C.cast(g.c, C.c_void_p),
         C.cast(g.p, C.c_void_p), dtype_enum(g.dtype), batch, _p(mask), S, int(l1), _s())


def masked_sse_all(g, batch, mask, S, img_a, lda, img_b, ldb, img_c, img_partial, l1=False):
    """masked_sse_multi(g, ...) and masked_sse_f32(img_a, lda, img_b, ldb, batch, S, img_c, mask, img_partial) in one launch."""
    call('imm_masked_sse_all', g.n, C.cast(g.a, C.c_void_p), C.cast(g.b, C.c_void_p), C.cast(g.s, C.c_void_p), C.cast(g.c, C.c_void_p),
         C.cast(g.p, C.c_void_p), dtype_enum(g.dtype), batch, _p(mask), S, int(l1), _p(img_a), lda, _p(img_b), ldb, img_c,
         _p(img_partial), _s())


def masked_sse_f32(a, lda, b, ldb, batch, s, c, mask, partial, l1=False):
    call('imm_masked_sse_f32', _p(a), lda, _p(b), ldb, batch, s, c, _p(mask), int(l1), _p(partial), _s())


LOSS_PERCEPTUAL, LOSS_L2 = 0, 1


def perceptual_finalize(partial, nfeat, nel, agg, training, wd_loss, out, l1=False, mode=LOSS_PERCEPTUAL, loss_scale=None):
    call('imm_perceptual_finalize', _p(partial), nfeat, _p(nel), _p(agg), int(training), _p(wd_loss), int(l1), int(mode),
         _p(loss_scale), _p(out), _s())


def tap_grad(da, has_in, a_pred, a_gt, batch, s, c, mask, S, coef, idx, relu, l1=False):
    call('imm_tap_grad', _p(da), int(has_in), _p(a_pred), _p(a_gt), dtype_enum(da.dtype), batch, s, c, _p(mask), S,
         _p(coef), idx, int(relu), int(l1), _s())


def copy_f32(dst, src):
    """dst <- src (f32, same numel) by a KERNEL on torch's current stream; either may be a pinned host tensor."""
    assert dst.dtype == torch.float32 and src.dtype == torch.float32 and dst.numel() == src.numel()
    assert dst.is_contiguous() and src.is_contiguous() and (dst.is_cuda or dst.is_pinned()) and (src.is_cuda or src.is_pinned())
    call('imm_copy_f32', _p(dst), _p(src), dst.numel(), _s())


def upload(dst, src, what='tensor'):
    """dst (device) <- src (host tensor / ndarray), staged through PINNED memory, stream-synchronised and read back: for the
    ONE-TIME transfers (initial parameters, frozen VGG weights, restored checkpoints).  Per-step inputs go through PinnedStager
    (no read-back, no full synchronisation).

    Why not `dst.copy_(cpu_tensor)`: with eight processes sharing one GPU, about once in 100 engine constructions ONE rank started
    from other initial weights in exactly the 2.4 MB / 2.9 MB filters — uploaded one by one from pageable temporaries that were freed
    (and refilled with the next tensor's random numbers) as soon as `copy_` returned (round 5; found by comparing the replicas'
    parameters before the first update — DESIGN.md §7; the runtime's pin-in-place path for pageable sources above ~1 MB is the
    inferred culprit).  Here the source is pinned (read in place by the DMA engine), the stream is synchronised before the staging
    buffer may go, and the result is read back and compared bitwise.  A mismatch RAISES (round 6: no silent repetition — with the
    cause removed a wrong read-back is a new bug and must be seen)."""
    if not dst.is_cuda:
        dst.copy_(torch.as_tensor(src).reshape(dst.shape))
        return
    src = torch.as_tensor(src)
    if src.is_cuda:
        dst.copy_(src.reshape(dst.shape))
        return
    stage = torch.empty(dst.shape, dtype=dst.dtype, pin_memory=True)
    stage.copy_(src.reshape(dst.shape))                    # host side: layout / dtype conversion into the pinned buffer
    back = torch.empty(dst.shape, dtype=dst.dtype, pin_memory=True)
    stream = torch.cuda.current_stream(dst.device)
    dst.copy_(stage, non_blocking=True)
    back.copy_(dst, non_blocking=True)
    stream.synchronize()
    if not torch.equal(back.reshape(-1).view(torch.uint8), stage.reshape(-1).view(torch.uint8)):
        nbad = int((back.reshape(-1).view(torch.uint8) != stage.reshape(-1).view(torch.uint8)).sum())
        raise RuntimeError('imm_amd: host-to-device upload of %s (%d bytes) does not read back as written (%d bytes differ)'
                           % (what, stage.numel() * stage.element_size(), nbad))


class PinnedStager:
    """Per-step host -> device copies (a training loop fed from host tensors: IMMEngine.set_inputs): every destination has TWO
    persistent pinned staging buffers, used alternately; a buffer is refilled only after the copy that last read it has finished
    (an event per buffer — two steps back, so in steady state the wait is free), the copy itself is asynchronous on the caller's
    stream: no allocation, no read-back, no stream-wide synchronisation per step, and the host side of step n + 1 overlaps the
    device side of step n (VERDICT r5 item 8 / ADVICE r5: the verified `upload` serialised a host-fed loop with the device)."""

    def __init__(self):
        self._slots = {}

    def copy(self, dst, src, key=None):
        src = torch.as_tensor(src)
        if not dst.is_cuda or src.is_cuda:
            dst.copy_(src.reshape(dst.shape))             # device -> device (the loader's / the bench's tensors): stream-ordered
            return
        key = dst.data_ptr() if key is None else key
        ent = self._slots.get(key)
        if ent is None or ent['bufs'][0].shape != dst.shape or ent['bufs'][0].dtype != dst.dtype:
            ent = {'bufs': [torch.empty(dst.shape, dtype=dst.dtype, pin_memory=True) for _ in range(2)], 'evs': [None, None], 'i': 0}
            self._slots[key] = ent
        i = ent['i']
        ent['i'] = 1 - i
        if ent['evs'][i] is not None:
            ent['evs'][i].synchronize()                   # the copy that read this buffer two calls ago
        ent['bufs'][i].copy_(src.reshape(dst.shape))      # host side: layout / dtype conversion into pinned memory
        dst.copy_(ent['bufs'][i], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dst.device))
        ent['evs'][i] = ev


def to_device_pinned(src, device, dtype=None):
    """A NEW device tensor holding `src` (host tensor / ndarray), copied from a pinned staging buffer that stays alive until the
    copy has finished (the host waits for THAT copy's event, not for the stream's earlier work).  What scripts and datasets use
    instead of `torch.from_numpy(x).to(device)`: a pageable temporary of more than ~1 MB that is freed right after `.to()` returns
    is the pattern behind round 5's torn upload (`upload` above); tests/test_host_cpu.py greps for it."""
    src = torch.as_tensor(src)
    device = torch.device(device)
    dtype = src.dtype if dtype is None else dtype
    if device.type != 'cuda' or src.is_cuda:
        return src.to(device=device, dtype=dtype)
    stage = torch.empty(src.shape, dtype=dtype, pin_memory=True)
    stage.copy_(src)
    dst = torch.empty(src.shape, dtype=dtype, device=device)
    dst.copy_(stage, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    ev.synchronize()
    return dst


def download(src):
    """Host copy of a device tensor through pinned memory, stream-synchronised (the mirror of upload(): checkpoints are written from
    these); returns an ordinary (pageable) CPU tensor."""
    if not src.is_cuda:
        return src.detach().clone()
    back = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
    back.copy_(src.detach(), non_blocking=True)
    torch.cuda.current_stream(src.device).synchronize()
    return back.clone()


def cost_ema(cost3, state4, decay=0.99):
    """BaseModel._add_cost_summary's moving averages (base_model.py:52-60): state4 = {biased[3], local_step}."""
    call('imm_cost_ema', _p(cost3), _p(state4), float(decay), _s())


def rms16(x, partial, out):
    """sqrt(mean(x^2)) of a contiguous 16-bit tensor (selfsup/vgg16.py:232-234 'activation/<layer>'); partial: f32 scratch."""
    assert x.is_contiguous() and x.numel() % 8 == 0
    call('imm_rms16', _p(x), x.numel(), dtype_enum(x.dtype), _p(partial), min(int(partial.numel()), 4096), _p(out), _s())


# ---- optimizer --------------------------------------------------------------------------------
def weight_decay_loss(params, tab, blk_partial, out):
    call('imm_weight_decay_loss', _p(params), _p(tab.blk_seg), _p(tab.blk_begin), _p(tab.blk_end), tab.nblk, _p(tab.seg_wd),
         _p(blk_partial), _p(out), _s())


def clip_adam_step(params, grads, m, v, tab, blk_partial, seg_norm2, step_count, adam_t, lr_state, hp, loss_scale_state=None):
    call('imm_clip_adam_step', _p(params), _p(grads), _p(m), _p(v), _p(tab.blk_seg), _p(tab.blk_begin), _p(tab.blk_end),
         tab.nblk, tab.nseg, _p(tab.seg_first_blk), _p(tab.seg_wd), _p(blk_partial), _p(seg_norm2), _p(step_count),
         _p(adam_t), _p(lr_state), C.byref(hp), _p(loss_scale_state), _s())


class SegmentTable:
    """Device-side description of the flat parameter buffer: tensors (segments) and the chunk each
    optimizer workgroup owns."""
    CHUNK = 2048     # 8192: 37 us for the update launch, 4096: 34, 2048: 32 (more 16-byte requests in flight per CU)

    def __init__(self, sizes, wds, device):
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + int(n))
        blk_seg, blk_begin, blk_end, first = [], [], [], [0]
        for s, n in enumerate(sizes):
            for b0 in range(0, int(n), self.CHUNK):
                blk_seg.append(s)
                blk_begin.append(offs[s] + b0)
                blk_end.append(offs[s] + min(int(n), b0 + self.CHUNK))
            first.append(len(blk_seg))
        self.offsets = offs
        self.nseg, self.nblk, self.total = len(sizes), len(blk_seg), offs[-1]
        i32 = dict(dtype=torch.int32, device=device)
        self.blk_seg = torch.tensor(blk_seg, **i32)
        self.blk_begin = torch.tensor(blk_begin, **i32)
        self.blk_end = torch.tensor(blk_end, **i32)
        self.seg_first_blk = torch.tensor(first, **i32)
        self.seg_wd = torch.tensor([float(w) for w in wds], dtype=torch.float32, device=device)


def debug_stamp(slots, index):
    """slots: int64 device tensor; slots[index] = device wall clock (100 MHz ticks) at this point of the current stream."""
    call('imm_debug_stamp', _p(slots), int(index), _s())


def _check_pixels(name, t, shape, c_min, ld=None):
    """t: an f32 NHWC tensor or view [shape..., >= c_min channels] whose pixels are dense at one stride: element (b, y, x, ch) at
    ((b * h + y) * w + x) * ld + ch floats, which is how the kernels address it (ld: the stride the call passes, t.stride(2) when
    None).  A ValueError that names the tensor otherwise; returns ld."""
    b, h, w = shape
    ld = t.stride(2) if ld is None and t.dim() == 4 else ld
    if (t.dtype != torch.float32 or t.dim() != 4 or t.shape[0] != b or tuple(t.shape[1:3]) != (h, w) or t.shape[3] < c_min or
            ld < t.shape[3] or any(n > 1 and st != want for n, st, want in zip(t.shape, t.stride(), (h * w * ld, w * ld, ld, 1)))):
        raise ValueError('%s must be f32 [%d, %d, %d, >= %d] with dense pixels of one stride%s, got %s %s strides %s' % (
            name, b, h, w, c_min, '' if ld is None else ' %d' % ld, t.dtype, tuple(t.shape), tuple(t.stride())))
    return ld


def _check_tps(src, basis_t, w_tps, grid_pixels):
    """The operands both TPS warps share -> (b, h, w, c, ld_src, m3)."""
    if src.dim() != 4:
        raise ValueError('src must be f32 [B, H, W, C], got %s %s' % (src.dtype, tuple(src.shape)))
    b, h, w, c = src.shape
    ld_src = _check_pixels('src', src, (b, h, w), c)
    m3 = w_tps.shape[1] if w_tps.dim() == 3 else -1
    _check_tensors([('w_tps', w_tps, torch.float32, (b, None, 2)), ('basis_t', basis_t, torch.float32, (m3, grid_pixels))])
    return b, h, w, c, ld_src, m3


def tps_warp(src, basis_t, w_tps, dst=None, dst_c0=None, dst_rest=None):
    """src [B,H,W,C] f32 NHWC; basis_t [M+3, H*W]; w_tps [B, M+3, 2]; outputs as in include/imm_hip.h (imm_tps_warp): dst [B,H,W,>=C],
    dst_c0 [B,H,W] (contiguous), dst_rest [B,H,W,>=C-1].  src, dst and dst_rest may be channel views of wider buffers (dense pixels of
    one stride).  ValueError before the launch for a tensor of another type, shape or layout."""
    b, h, w, c, ld_src, m3 = _check_tps(src, basis_t, w_tps, src.shape[1] * src.shape[2] if src.dim() == 4 else 0)
    c_out = c if 1 <= c <= 8 else 0          # c out of range is the library's refusal
    ld_dst = _check_pixels('dst', dst, (b, h, w), c_out) if dst is not None else 0
    ld_rest = _check_pixels('dst_rest', dst_rest, (b, h, w), max(c_out - 1, 0)) if dst_rest is not None else 0
    if dst_c0 is not None:
        _check_tensors([('dst_c0', dst_c0, torch.float32, (b, h, w))])
    call('imm_tps_warp', _p(src), ld_src, b, h, w, c, _p(basis_t), m3, _p(w_tps), _p(dst), ld_dst, _p(dst_c0), _p(dst_rest), ld_rest, _s())


def tps_warp_pad(src, basis_t, w_tps, pad_yx, grid_hw, crop_yx, dst):
    """TPSRandomSampler(pad=True): src [B,H,W,C] f32 NHWC read as if replicate-padded by pad_yx, warped on a grid_hw grid
    (basis_t [M+3, gh*gw]), window crop_yx + dst.shape[1:3] written to dst [B,oh,ow,>=C] (include/imm_hip.h: imm_tps_warp_pad).
    ValueError before the launch for a tensor of another type, shape or layout."""
    b, h, w, c, ld_src, m3 = _check_tps(src, basis_t, w_tps, int(grid_hw[0]) * int(grid_hw[1]))
    if dst.dim() != 4:
        raise ValueError('dst must be f32 [B, oh, ow, >= C], got %s %s' % (dst.dtype, tuple(dst.shape)))
    ld_dst = _check_pixels('dst', dst, (b, dst.shape[1], dst.shape[2]), c if 1 <= c <= 8 else 0)
    call('imm_tps_warp_pad', _p(src), ld_src, b, h, w, c, pad_yx[0], pad_yx[1], grid_hw[0], grid_hw[1], crop_yx[0], crop_yx[1],
         dst.shape[1], dst.shape[2], _p(basis_t), m3, _p(w_tps), _p(dst), ld_dst, _s())


def resize_crop_u8(src_u8, offsets, hw, c, resize_hw, crop_yx, out_hw, dst, ld_dst=None, boxes=None):
    """src_u8: flat u8 device buffer of packed HWC images; offsets i64 [images]; hw i32 [images, 2]; dst f32 [>= batch, oh, ow, >= c],
    a tensor or a channel view of a wider buffer, whose element (b,y,x,0) is dst.data_ptr() + ((b*oh+y)*ow+x)*ld_dst floats
    (include/imm_hip.h: imm_resize_crop_u8; rows of dst beyond batch are left alone).
    boxes: None, or int32 [n, 5] device rows (image, y0, x0, y1, x1) checked on the host beforehand
    (imm_amd.keypoints.check_boxes): output row b is box b cut from its image, zero-padded, then resized and cropped.
    ValueError before the launch for a tensor of another type, shape or layout."""
    if boxes is not None and (boxes.dtype != torch.int32 or boxes.dim() != 2 or boxes.shape[1] != 5 or not boxes.is_contiguous()):
        raise ValueError('boxes must be contiguous int32 [n, 5], got %s %s' % (boxes.dtype, tuple(boxes.shape)))
    _check_tensors([('src_u8', src_u8, torch.uint8, (None,)), ('hw', hw, torch.int32, (None, 2))])
    _check_tensors([('offsets', offsets, torch.int64, (hw.shape[0],))])
    batch = hw.shape[0] if boxes is None else boxes.shape[0]
    if dst.dim() != 4 or dst.shape[0] < batch:
        raise ValueError('dst must be f32 [>= %d, %d, %d, >= c], got %s %s' % (batch, out_hw[0], out_hw[1], dst.dtype, tuple(dst.shape)))
    # (c out of range is the library's refusal)
    ld_dst = _check_pixels('dst', dst, (dst.shape[0], int(out_hw[0]), int(out_hw[1])), c if 1 <= c <= 4 else 0, ld_dst)
    call('imm_resize_crop_u8', _p(src_u8), _p(offsets), _p(hw), _p(boxes), batch, c, resize_hw[0], resize_hw[1], crop_yx[0],
         crop_yx[1], out_hw[0], out_hw[1], _p(dst), ld_dst, _s())


MAX_ALIGN_M3 = 67             # basis functions of an alignment map: K <= 64 radial ones + 1, q_y, q_x


def align_coeffs(mu, ft, k, m3, coef):
    """coef f32 [n, m3, 2] = F . vec(mu) per row; mu f32 [n, K, 2]; ft f32 [2K, 2 m3] = F transposed (include/imm_align.h:
    imm_align_coeffs)."""
    if ft.dtype != torch.float32 or ft.numel() != 4 * k * m3 or not ft.is_contiguous():
        raise ValueError('ft must be contiguous f32 [2K, 2 m3] = [%d, %d], got %s %s' % (2 * k, 2 * m3, ft.dtype, tuple(ft.shape)))
    n = mu.shape[0]
    assert mu.is_contiguous() and coef.is_contiguous() and mu.numel() == n * 2 * k and coef.numel() == n * 2 * m3
    call('imm_align_coeffs', _p(mu), _p(ft), n, int(k), int(m3), _p(coef), _s())


def align_warp_u8(src, offsets, hw, boxes, geom, coef, basis_t, image_size, dst, ld_dst=None):
    """dst f32 [n, So, So, >= 3]: every row's photo sampled once through its map and geometry (include/imm_align.h: imm_align_warp_u8).
    src: the packed u8 buffer with offsets i64 [images], hw i32 [images, 2] and boxes i32 [n, 5] (as resize_crop_u8 takes them), or an
    f32 tensor [n, S, S, 3] with offsets = hw = boxes = None.  geom f32 [n, 4]; coef f32 [n, m3, 2]; basis_t f32 [m3, So * So] or None
    (m3 == 3)."""
    n, So = dst.shape[0], dst.shape[1]
    m3 = coef.shape[1]
    f32 = src.dtype == torch.float32
    if f32:
        if tuple(src.shape) != (n, image_size, image_size, 3) or not src.is_contiguous():
            raise ValueError('an f32 source must be contiguous [n, S, S, 3], got %s' % (tuple(src.shape),))
        n_images = n
    else:
        if src.dtype != torch.uint8 or offsets is None or hw is None or boxes is None:
            raise ValueError('a u8 source needs offsets, hw and boxes')
        if boxes.dtype != torch.int32 or tuple(boxes.shape) != (n, 5) or not boxes.is_contiguous():
            raise ValueError('boxes must be contiguous int32 [n, 5], got %s %s' % (boxes.dtype, tuple(boxes.shape)))
        n_images = hw.shape[0]
    if dst.shape[2] != So or tuple(geom.shape) != (n, 4) or tuple(coef.shape) != (n, m3, 2) or not (geom.is_contiguous() and coef.is_contiguous()):
        raise ValueError('dst [n, So, So, c], geom [n, 4], coef [n, m3, 2] (contiguous)')
    if (m3 > 3) != (basis_t is not None) or (basis_t is not None and (tuple(basis_t.shape) != (m3, So * So) or not basis_t.is_contiguous())):
        raise ValueError('basis_t must be contiguous f32 [m3, So * So] for m3 > 3 and None for m3 == 3')
    call('imm_align_warp_u8', _p(src), int(f32), _p(offsets), _p(hw), int(n_images), _p(boxes), _p(geom), _p(coef), _p(basis_t), int(m3),
         n, int(image_size), So, _p(dst), dst.stride(2) if ld_dst is None else ld_dst, _s())


def _check_tensors(specs):
    """(name, tensor, dtype, shape) each: a ValueError that names the first tensor that is not contiguous with that dtype and shape; a
    dimension given as None is free (hw i32 [images, 2], a flat packed buffer u8 [bytes])."""
    for name, t, dt, shape in specs:
        if (t.dtype != dt or t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)) or
                not t.is_contiguous()):
            raise ValueError('%s must be contiguous %s [%s], got %s %s' % (name, str(dt).replace('torch.', ''), ', '.join(
                'any' if s is None else str(s) for s in shape), t.dtype, tuple(t.shape)))


def _check_faces(faces, n):
    """faces f32 [n, S, S, >= 3] with dense pixels of one stride -> (S, that stride)."""
    S, ld = faces.shape[1], faces.stride(2)
    if (faces.dtype != torch.float32 or faces.dim() != 4 or faces.shape[0] != n or faces.shape[2] != S or faces.shape[3] < 3 or
            faces.stride(3) != 1 or faces.stride(1) != S * ld or faces.stride(0) != S * S * ld):
        raise ValueError('faces must be f32 [n, S, S, >= 3] with dense pixels of one stride, got %s %s strides %s' % (
            faces.dtype, tuple(faces.shape), tuple(faces.stride())))
    return S, ld


def compose_u8(photos, offsets, hw, boxes, links, inv_ramp, faces, max_box_pixels):
    """The packed u8 photos (as resize_crop_u8 reads them) composited in place: row b's face, faces[b] f32 [S, S, >= 3] (a view of
    any pixel stride, channels 0..2 read), resampled to box b, blended with the edge ramp inv_ramp f32 [n, 2] and rounded to u8, in
    row order (include/imm_compose.h: imm_compose_u8).  boxes i32 [n, 5], links i32 [n, 2] (generation.compose_links of THESE rows);
    max_box_pixels: the largest box area of the rows."""
    n = boxes.shape[0]
    _check_tensors([('photos', photos, torch.uint8, (None,)), ('boxes', boxes, torch.int32, (n, 5)), ('links', links, torch.int32, (n, 2)),
                    ('inv_ramp', inv_ramp, torch.float32, (n, 2))])
    S, ld = _check_faces(faces, n)
    call('imm_compose_u8', _p(photos), _p(offsets), _p(hw), int(hw.shape[0]), _p(boxes), _p(links), _p(inv_ramp), _p(faces), int(ld), n,
         int(S), int(max_box_pixels), _s())


def unalign_maps(coef, geom, boxes, hw, image_size, out_size, fwd, bbox):
    """fwd f32 [n, 6] (photo pixel -> aligned coordinate, m00 m01 m02 m10 m11 m12) and bbox i32 [n, 4] (half-open, in the row's photo)
    from the backward maps of align(): coef f32 [n, 3, 2], geom f32 [n, 4], boxes i32 [n, 5] (the image index is read), hw i32
    [images, 2] (include/imm_unalign.h: imm_unalign_maps).  Everything stays on the device."""
    n = boxes.shape[0]
    # coef [n, 3, 2]: the similarity and affine models
    _check_tensors([('boxes', boxes, torch.int32, (n, 5)), ('coef', coef, torch.float32, (n, 3, 2)), ('geom', geom, torch.float32, (n, 4)),
                    ('hw', hw, torch.int32, (None, 2)), ('fwd', fwd, torch.float32, (n, 6)), ('bbox', bbox, torch.int32, (n, 4))])
    call('imm_unalign_maps', _p(coef), _p(geom), _p(boxes), _p(hw), int(hw.shape[0]), n, int(image_size), int(out_size), _p(fwd),
         _p(bbox), _s())


def unalign_u8(photos, offsets, hw, boxes, links, fwd, bbox, inv_ramp, faces, max_pixels):
    """The packed u8 photos (as resize_crop_u8 reads them) pasted into in place: row b's aligned face, faces[b] f32 [So, So, >= 3] (a
    view of any pixel stride, channels 0..2 read), sampled through fwd[b] at every photo pixel of bbox[b] the map covers, blended with
    the edge ramp of reciprocal width inv_ramp (a float) and rounded to u8, in row order (include/imm_unalign.h: imm_unalign_u8).
    boxes i32 [n, 5] (the image index is read), links i32 [n, 2] (generation.compose_links of THESE rows), fwd f32 [n, 6] and bbox i32
    [n, 4] from unalign_maps; max_pixels: the largest bbox area expected (it sizes the grid only)."""
    n = boxes.shape[0]
    _check_tensors([('photos', photos, torch.uint8, (None,)), ('boxes', boxes, torch.int32, (n, 5)), ('links', links, torch.int32, (n, 2)),
                    ('fwd', fwd, torch.float32, (n, 6)), ('bbox', bbox, torch.int32, (n, 4))])
    So, ld = _check_faces(faces, n)
    call('imm_unalign_u8', _p(photos), _p(offsets), _p(hw), int(hw.shape[0]), _p(boxes), _p(links), _p(fwd), _p(bbox), float(inv_ramp),
         _p(faces), int(ld), n, int(So), int(max_pixels), _s())


def track_step(mu, boxes, hw, state, image_size, next_image, init, box_smooth, min_cutoff, beta, d_cutoff, c, te, filter_off, points,
               points_smooth, boxes_next, geom_next, flags):
    """One frame of face tracking (include/imm_track.h: imm_track_step): mu f32 [F, K, 2] and the rows boxes i32 [F, 5] this frame was
    cut with -> points, points_smooth f32 [F, K, 2] (source pixels), the next frame's rows boxes_next i32 [F, 5] (image index
    next_image) with their geometry geom_next f32 [F, 4], and flags i32 [F]; state f64 [F, 5 + 6 K] (tracking.state_size) is read
    and written.  hw i32 [images, 2]: the sizes of the photos `boxes` index.  c = 2 pi / fps and te = 1 / fps come from the host."""
    F, K = mu.shape[0], mu.shape[1]
    _check_tensors([('mu', mu, torch.float32, (F, K, 2)), ('boxes', boxes, torch.int32, (F, 5)), ('state', state, torch.float64, (F, 5 + 6 * K)),
                    ('points', points, torch.float32, (F, K, 2)), ('points_smooth', points_smooth, torch.float32, (F, K, 2)),
                    ('boxes_next', boxes_next, torch.int32, (F, 5)), ('geom_next', geom_next, torch.float32, (F, 4)),
                    ('flags', flags, torch.int32, (F,)), ('hw', hw, torch.int32, (None, 2))])
    call('imm_track_step', _p(mu), _p(boxes), _p(hw), _p(state), int(K), int(image_size), int(F), int(hw.shape[0]), int(next_image),
         int(init), float(box_smooth), float(min_cutoff), float(beta), float(d_cutoff), float(c), float(te), int(bool(filter_off)),
         _p(points), _p(points_smooth), _p(boxes_next), _p(geom_next), _p(flags), _s())


def landmark_scores(py, px, mu, boxes, ref, ref_stride, image_size, max_spread, max_residual, blank, spread, score, qflags, mu_out):
    """The quality scores of F faces (include/imm_score.h: imm_landmark_scores): the soft-argmax marginals py f32 [F, h, K], px f32
    [F, w, K] and the landmarks mu f32 [F, K, 2] -> spread f32 [F, K], score f32 [F, 2] = (mean spread, shape residual), qflags i32 [F]
    (bit 0: the spread fails max_spread, bit 1: the residual fails max_residual; None or +inf: not applied) and mu_out f32 [F, K, 2] (mu's
    bits, NaN for a flagged face with blank; None allowed without blank).  boxes i32 [F, 5] or None: the rows the faces were cut with
    (the residual is then taken in source pixels).  ref: a contiguous f64 tensor holding the reference shape [K, 2] of face f at element
    f * ref_stride (ref_stride 0: one shape for all), or None (residual 0)."""
    if mu.dim() != 3 or py.dim() != 3 or px.dim() != 3:
        raise ValueError('py [F, h, K], px [F, w, K], mu [F, K, 2], got %s, %s, %s' % (tuple(py.shape), tuple(px.shape), tuple(mu.shape)))
    F, K, h, w = int(mu.shape[0]), int(mu.shape[1]), int(py.shape[1]), int(px.shape[1])
    specs = [('py', py, torch.float32, (F, h, K)), ('px', px, torch.float32, (F, w, K)), ('mu', mu, torch.float32, (F, K, 2)),
             ('spread', spread, torch.float32, (F, K)), ('score', score, torch.float32, (F, 2)), ('qflags', qflags, torch.int32, (F,))]
    if boxes is not None:
        specs.append(('boxes', boxes, torch.int32, (F, 5)))
    if mu_out is not None:
        specs.append(('mu_out', mu_out, torch.float32, (F, K, 2)))
    if ref is not None:
        specs.append(('ref', ref, torch.float64, tuple(None for _ in ref.shape)))
    _check_tensors(specs)
    ref_stride = int(ref_stride) if ref is not None else 0
    if ref is not None and not (ref_stride == 0 or ref_stride >= 2 * K) or (
            ref is not None and ref.numel() < (F - 1) * ref_stride + 2 * K):
        raise ValueError('ref must hold 2 K doubles per face at a stride of 0 or >= 2 K, got %d values at stride %d for F = %d, K = %d' % (
            ref.numel(), ref_stride, F, K))
    if mu_out is not None and _overlap(mu, mu_out):
        raise ValueError('mu overlaps mu_out: the output is written while the input is read')
    inf = float('inf')
    call('imm_landmark_scores', _p(py), _p(px), _p(mu), _p(boxes), _p(ref), ref_stride, K, h, w, int(image_size), F,
         inf if max_spread is None else float(max_spread), inf if max_residual is None else float(max_residual), int(blank),
         _p(spread), _p(score), _p(qflags), _p(mu_out), _s())


def retarget(q, anchor, driver_flags, m, prev, init, relative, rigid, gain, out, flags):
    """One frame of re-enactment (include/imm_retarget.h: imm_retarget): the driver's points q f32 [K, 2] of this frame, the anchor f64
    [K, 2] (set to q with init) and the driver's track_step flags i32 [1] -> the poses out f32 [n, K, 2] of the source faces with the
    landmarks m f32 [n, K, 2], and flags i32 [n] (bit 0: held, out = prev f32 [n, K, 2]).  out may be prev."""
    n, K = m.shape[0], m.shape[1]
    _check_tensors([('q', q, torch.float32, (K, 2)), ('anchor', anchor, torch.float64, (K, 2)), ('driver_flags', driver_flags, torch.int32, (1,)),
                    ('m', m, torch.float32, (n, K, 2)), ('prev', prev, torch.float32, (n, K, 2)), ('out', out, torch.float32, (n, K, 2)),
                    ('flags', flags, torch.int32, (n,))])
    call('imm_retarget', _p(q), _p(anchor), _p(driver_flags), _p(m), _p(prev), int(K), int(n), int(init), int(bool(relative)),
         int(bool(rigid)), float(gain), _p(out), _p(flags), _s())


WARP_MAX_POINTS = 80          # control points of a warp spline: landmarks + border anchors


def warp_fit(poses, mu, anchors, strength, lam, coef, ctrl, flags):
    """The per-face thin-plate spline of LandmarkDetector.warp (include/imm_warp.h: imm_warp_fit): poses f32 [n, K, 2] (the target
    landmarks) and mu f32 [n, K, 2] (the faces' own) with the border anchors f32 [A, 2] (None or empty: no anchors) -> coef f32
    [n, K + A + 3, 2], ctrl f32 [n, K + A, 2] and flags i32 [n] (bit 0: no usable fit, the row's coefficients are NaN)."""
    if poses.dim() != 3 or poses.shape[2] != 2:
        raise ValueError('poses must be f32 [n, K, 2], got %s' % (tuple(poses.shape),))
    n, K = int(poses.shape[0]), int(poses.shape[1])
    A = 0 if anchors is None else int(anchors.shape[0])
    M = K + A
    if n < 1 or n > 65535 or K < 1 or A % 4 or not 3 <= M <= WARP_MAX_POINTS:
        raise ValueError('warp_fit serves 1..65535 rows of K >= 1 landmarks and A = 4 m anchors with 3 <= K + A <= %d, got n = %d, K = %d, '
                         'A = %d' % (WARP_MAX_POINTS, n, K, A))
    specs = [('poses', poses, torch.float32, (n, K, 2)), ('mu', mu, torch.float32, (n, K, 2)), ('coef', coef, torch.float32, (n, M + 3, 2)),
             ('ctrl', ctrl, torch.float32, (n, M, 2)), ('flags', flags, torch.int32, (n,))]
    if A:
        specs.append(('anchors', anchors, torch.float32, (A, 2)))
    _check_tensors(specs)
    strength, lam = float(strength), float(lam)
    if strength - strength != 0.0:
        raise ValueError('strength must be finite, got %r' % (strength,))
    if not (lam >= 0.0 and lam - lam == 0.0):
        raise ValueError('lam must be finite and >= 0, got %r' % (lam,))
    call('imm_warp_fit', _p(poses), _p(mu), _p(anchors) if A else None, K, A, n, strength, lam, _p(coef), _p(ctrl), _p(flags), _s())


def warp_u8(src, dst, offsets, hw, boxes, links, inv_ramp, ctrl, coef, max_box_pixels):
    """The packed u8 photos dst (a copy of src, as resize_crop_u8 reads them) warped in place: every pixel of row b's box takes the
    ORIGINAL photo's (src, read only) value at the place the row's spline (ctrl f32 [n, M, 2], coef f32 [n, M + 3, 2] from warp_fit)
    sends it to, blended with the edge ramp inv_ramp f32 [n, 2] and rounded to u8, in row order (include/imm_warp.h: imm_warp_u8).
    boxes i32 [n, 5], links i32 [n, 2] (generation.compose_links of THESE rows); max_box_pixels: the largest box area of the rows."""
    if boxes.dim() != 2 or ctrl.dim() != 3:
        raise ValueError('boxes must be int32 [n, 5] and ctrl f32 [n, M, 2], got %s and %s' % (tuple(boxes.shape), tuple(ctrl.shape)))
    n, M = int(boxes.shape[0]), int(ctrl.shape[1])
    _check_tensors([('src', src, torch.uint8, (None,)), ('dst', dst, torch.uint8, (None,))])
    if src.numel() != dst.numel() or src.data_ptr() == dst.data_ptr():
        raise ValueError('dst must be a copy of src (same size, another buffer): every row samples the original pixels')
    if n < 1 or n > 65535 or not 3 <= M <= WARP_MAX_POINTS:
        raise ValueError('warp_u8 serves 1..65535 rows of 3 <= M <= %d control points, got n = %d, M = %d' % (WARP_MAX_POINTS, n, M))
    _check_tensors([('boxes', boxes, torch.int32, (n, 5)), ('links', links, torch.int32, (n, 2)), ('inv_ramp', inv_ramp, torch.float32, (n, 2)),
                    ('ctrl', ctrl, torch.float32, (n, M, 2)), ('coef', coef, torch.float32, (n, M + 3, 2)),
                    ('hw', hw, torch.int32, (None, 2)), ('offsets', offsets, torch.int64, (hw.shape[0],))])
    if int(max_box_pixels) < 1:
        raise ValueError('max_box_pixels must be positive, got %r' % (max_box_pixels,))
    call('imm_warp_u8', _p(src), _p(dst), _p(offsets), _p(hw), int(hw.shape[0]), _p(boxes), _p(links), _p(inv_ramp), _p(ctrl), _p(coef), M, n,
         int(max_box_pixels), _s())


MORPH_MAX_ROWS = 32767        # rows of one morph: the fit that follows imm_morph_poses takes twice as many


def morph_poses(mu_a, mu_b, shape, poses2, mu2):
    """The pose blend of LandmarkDetector.morph (include/imm_morph.h: imm_morph_poses): mu_a, mu_b f32 [n, K, 2] (the faces' own and
    their donors' landmarks) and shape f32 [n] -> poses2 f32 [2, n, K, 2] (p = (1 - s) mu_a + s mu_b, twice) and mu2 f32 [2, n, K, 2]
    ((mu_a, mu_b)): viewed as [2 n, K, 2], the poses and mu of ONE warp_fit over 2 n rows."""
    if mu_a.dim() != 3 or mu_a.shape[2] != 2:
        raise ValueError('mu_a must be f32 [n, K, 2], got %s' % (tuple(mu_a.shape),))
    n, K = int(mu_a.shape[0]), int(mu_a.shape[1])
    if n < 1 or n > MORPH_MAX_ROWS or K < 1 or K > WARP_MAX_POINTS:
        raise ValueError('morph_poses serves 1..%d rows of 1..%d landmarks, got n = %d, K = %d' % (MORPH_MAX_ROWS, WARP_MAX_POINTS, n, K))
    _check_tensors([('mu_a', mu_a, torch.float32, (n, K, 2)), ('mu_b', mu_b, torch.float32, (n, K, 2)), ('shape', shape, torch.float32, (n,)),
                    ('poses2', poses2, torch.float32, (2, n, K, 2)), ('mu2', mu2, torch.float32, (2, n, K, 2))])
    for name, t in (('mu_a', mu_a), ('mu_b', mu_b), ('shape', shape)):
        for oname, o in (('poses2', poses2), ('mu2', mu2)):
            if _overlap(t, o):
                raise ValueError('%s overlaps %s: the outputs are written while the inputs are read' % (name, oname))
    if _overlap(poses2, mu2):
        raise ValueError('poses2 overlaps mu2')
    call('imm_morph_poses', _p(mu_a), _p(mu_b), _p(shape), K, n, _p(poses2), _p(mu2), _s())


def _overlap(a, b):
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _check_photos(src, offsets, hw, donor, donor_offsets, donor_hw):
    """The packed photo and donor buffers as morph_paste and seam_fit read them: src and donor u8 [bytes], hw and donor_hw i32 [images, 2]
    of at least one image each, offsets and donor_offsets i64, one per image."""
    _check_tensors([('src', src, torch.uint8, (None,)), ('donor', donor, torch.uint8, (None,)), ('hw', hw, torch.int32, (None, 2)),
                    ('donor_hw', donor_hw, torch.int32, (None, 2))])
    if hw.shape[0] < 1 or donor_hw.shape[0] < 1:
        raise ValueError('hw and donor_hw must hold at least one image, got %s and %s' % (tuple(hw.shape), tuple(donor_hw.shape)))
    _check_tensors([('offsets', offsets, torch.int64, (hw.shape[0],)), ('donor_offsets', donor_offsets, torch.int64, (donor_hw.shape[0],))])


def _need(name, **args):
    """The arguments that define a named paste entry, as keywords of morph_paste: a ValueError names the first that is None."""
    for k, t in args.items():
        if t is None:
            raise ValueError('%s needs %s, got None' % (name, k))
    return args


def morph_paste(src, dst, offsets, hw, donor, donor_offsets, donor_hw, boxes, donor_boxes, links, inv_ramp, texture, ctrl, coef_a, coef_b,
                max_box_pixels, gain=None, edges=None, inv_soft=None, ring=None, diff=None, seamless=None):
    """The paste of LandmarkDetector.morph, every check made once and the entry point chosen by what is given, as morph_launch chooses
    the kernel's instantiation: ring (with diff and seamless; needs edges) -> imm_morph_seam_u8, else edges (with inv_soft) ->
    imm_morph_hull_u8, else gain -> imm_morph_colour_u8, else imm_morph_u8.  The sixteen leading arguments as morph_u8 takes them, the
    optional ones as morph_colour_u8, morph_hull_u8 and morph_seam_u8 do; none of them may overlap dst."""
    name = 'morph_seam_u8' if ring is not None else 'morph_hull_u8' if edges is not None else 'morph_colour_u8' if gain is not None else 'morph_u8'
    if boxes.dim() != 2 or ctrl.dim() != 3:
        raise ValueError('boxes must be int32 [n, 5] and ctrl f32 [n, M, 2], got %s and %s' % (tuple(boxes.shape), tuple(ctrl.shape)))
    n, M = int(boxes.shape[0]), int(ctrl.shape[1])
    _check_photos(src, offsets, hw, donor, donor_offsets, donor_hw)
    _check_tensors([('dst', dst, torch.uint8, (None,))])
    if src.numel() != dst.numel() or _overlap(src, dst):
        raise ValueError('dst must be a copy of src (same size, another buffer): every row samples the original pixels')
    if _overlap(donor, dst):
        raise ValueError('the donor buffer is read only: it may be src, never dst')
    if n < 1 or n > 65535 or not 3 <= M <= WARP_MAX_POINTS:
        raise ValueError('%s serves 1..65535 rows of 3 <= M <= %d control points, got n = %d, M = %d' % (name, WARP_MAX_POINTS, n, M))
    _check_tensors([('boxes', boxes, torch.int32, (n, 5)), ('donor_boxes', donor_boxes, torch.int32, (n, 5)), ('links', links, torch.int32, (n, 2)),
                    ('inv_ramp', inv_ramp, torch.float32, (n, 2)), ('texture', texture, torch.float32, (n,)),
                    ('ctrl', ctrl, torch.float32, (n, M, 2)), ('coef_a', coef_a, torch.float32, (n, M + 3, 2)),
                    ('coef_b', coef_b, torch.float32, (n, M + 3, 2))])
    if int(max_box_pixels) < 1:
        raise ValueError('max_box_pixels must be positive, got %r' % (max_box_pixels,))
    extra = dict(gain=gain, edges=edges, inv_soft=inv_soft, ring=ring, diff=diff, seamless=seamless)
    for group in (('edges', 'inv_soft'), ('ring', 'diff', 'seamless')):
        absent = [k for k in group if extra[k] is None]
        if absent and len(absent) < len(group):
            raise ValueError('%s come together: %s is None' % (' and '.join(group), absent[0]))
    if ring is not None and edges is None:
        raise ValueError('ring, diff and seamless need the mask they are fitted to: edges is None')
    # the 17 arguments every entry starts with, then what the chosen one adds: pointers, then sizes
    args = [_p(src), _p(dst), _p(offsets), _p(hw), int(hw.shape[0]), _p(donor), _p(donor_offsets), _p(donor_hw), int(donor_hw.shape[0]),
            _p(boxes), _p(donor_boxes), _p(links), _p(inv_ramp), _p(texture), _p(ctrl), _p(coef_a), _p(coef_b)]
    sizes = [M]
    if gain is not None:
        _check_tensors([('gain', gain, torch.float32, (n, 3, 2))])
    if name != 'morph_u8':
        args.append(_p(gain))
    if edges is not None:
        if edges.dim() != 3 or not 1 <= int(edges.shape[1]) <= WARP_MAX_POINTS:
            raise ValueError('edges must be f32 [n, K, 3] with 1 <= K <= %d, got %s' % (WARP_MAX_POINTS, tuple(edges.shape)))
        K = int(edges.shape[1])
        _check_tensors([('edges', edges, torch.float32, (n, K, 3)), ('inv_soft', inv_soft, torch.float32, (n,))])
        args += [_p(edges), _p(inv_soft)]
        sizes = [K, M]
    if ring is not None:
        B = _check_seam(ring, diff, n, name)
        _check_tensors([('seamless', seamless, torch.float32, (n,))])
        args += [_p(ring), _p(diff), _p(seamless)]
        sizes = [K, M, B]
    for k, t in extra.items():
        if t is not None and _overlap(t, dst):
            raise ValueError('%s overlaps dst' % k)
    call('imm_' + name, *args, *sizes, n, int(max_box_pixels), _s())


def morph_u8(src, dst, offsets, hw, donor, donor_offsets, donor_hw, boxes, donor_boxes, links, inv_ramp, texture, ctrl, coef_a, coef_b,
             max_box_pixels):
    """The packed u8 photos dst (a copy of src) morphed in place (include/imm_morph.h: imm_morph_u8): every pixel of row b's box takes
    the mix, by texture f32 [n], of the ORIGINAL photo's value (src, read only) at the place the row's spline coef_a sends it to and of
    the donor photo's value (donor, a second packed buffer with donor_offsets / donor_hw, read only; it may be src) at the place coef_b
    sends it to inside the donor box (donor_boxes i32 [n, 5]), blended with the edge ramp inv_ramp f32 [n, 2] and rounded to u8, in row
    order.  ctrl f32 [n, M, 2], coef_a / coef_b f32 [n, M + 3, 2]: the halves of ONE warp_fit over the 2 n rows of morph_poses.  boxes,
    links, max_box_pixels as warp_u8 takes them."""
    morph_paste(src, dst, offsets, hw, donor, donor_offsets, donor_hw, boxes, donor_boxes, links, inv_ramp, texture, ctrl, coef_a, coef_b,
                max_box_pixels)


COLOUR_MAX_AREA = 1 << 30     # H * W of a box whose pixels imm_colour_stats_u8 counts: the ellipse test stays inside 64 bits


def colour_stats_u8(buf, offsets, hw, boxes, max_box_pixels, sums):
    """The colour statistics of every row's region (include/imm_colour.h: imm_colour_stats_u8): buf u8 [bytes] with offsets i64 [images]
    and hw i32 [images, 2] (a packed buffer, as morph_u8 reads it) and boxes i32 [n, 5] -> sums i64 [n, 7], read as unsigned: per row the
    sums of v per channel, of v * v per channel and the pixel count over the pixels of the box that lie in the photo and in the ellipse
    inscribed in the box.  sums is cleared on the stream first.  max_box_pixels sizes the grid only."""
    if boxes.dim() != 2:
        raise ValueError('boxes must be int32 [n, 5], got %s' % (tuple(boxes.shape),))
    n = int(boxes.shape[0])
    if n < 1 or n > 65535:
        raise ValueError('colour_stats_u8 serves 1..65535 rows, got n = %d' % n)
    _check_tensors([('buf', buf, torch.uint8, (None,)), ('hw', hw, torch.int32, (None, 2))])
    if hw.shape[0] < 1:
        raise ValueError('hw must hold at least one image, got %s' % (tuple(hw.shape),))
    _check_tensors([('boxes', boxes, torch.int32, (n, 5)), ('offsets', offsets, torch.int64, (hw.shape[0],)), ('sums', sums, torch.int64, (n, 7))])
    if int(max_box_pixels) < 1:
        raise ValueError('max_box_pixels must be positive, got %r' % (max_box_pixels,))
    call('imm_colour_stats_u8', _p(buf), _p(offsets), _p(hw), int(hw.shape[0]), _p(boxes), n, int(min(int(max_box_pixels), 2 ** 31 - 1)),
         _p(sums), _s())


def colour_gain(sums_a, sums_b, amount, max_gain, gain, flags):
    """The gain and offset per row and channel (include/imm_colour.h: imm_colour_gain): sums_a, sums_b i64 [n, 7] (colour_stats_u8 of the
    faces and of their donors) and amount f32 [n] -> gain f32 [n, 3, 2] ((G, O) per channel) and flags i32 [n] (bit 0: a region without
    pixels or an amount that is not finite, the row got (1, 0)).  max_gain: finite, >= 1; the ratio of the spreads is clamped to
    [1 / max_gain, max_gain]."""
    if sums_a.dim() != 2:
        raise ValueError('sums_a must be int64 [n, 7], got %s' % (tuple(sums_a.shape),))
    n = int(sums_a.shape[0])
    if n < 1 or n > 65535:
        raise ValueError('colour_gain serves 1..65535 rows, got n = %d' % n)
    _check_tensors([('sums_a', sums_a, torch.int64, (n, 7)), ('sums_b', sums_b, torch.int64, (n, 7)), ('amount', amount, torch.float32, (n,)),
                    ('gain', gain, torch.float32, (n, 3, 2)), ('flags', flags, torch.int32, (n,))])
    max_gain = float(max_gain)
    if not (max_gain >= 1.0 and max_gain - max_gain == 0.0):
        raise ValueError('max_gain must be finite and >= 1, got %r' % (max_gain,))
    call('imm_colour_gain', _p(sums_a), _p(sums_b), _p(amount), max_gain, n, _p(gain), _p(flags), _s())


def morph_colour_u8(src, dst, offsets, hw, donor, donor_offsets, donor_hw, boxes, donor_boxes, links, inv_ramp, texture, ctrl, coef_a, coef_b,
                    gain, max_box_pixels):
    """morph_u8 with the donor's sample taken through gain f32 [n, 3, 2] (colour_gain's output for these rows) in front of the mix:
    gB * G + O per channel (include/imm_colour.h: imm_morph_colour_u8).  Every other argument as morph_u8 takes it."""
    morph_paste(src, dst, offsets, hw, donor, donor_offsets, donor_hw, boxes, donor_boxes, links, inv_ramp, texture, ctrl, coef_a, coef_b,
                max_box_pixels, **_need('morph_colour_u8', gain=gain))


def hull_fit(poses, boxes, grow, edges, flags):
    """The supporting lines of every row's grown landmark hull (include/imm_hull.h: imm_hull_fit): poses f32 [n, K, 2] (the target
    landmarks in the frame of the row's box; a contiguous view, e.g. the first half of morph_poses' poses2), boxes i32 [n, 5] and grow
    f32 [n] -> edges f32 [n, K, 3] ((ny, nx, d) per slot) and flags i32 [n] (bit 0: an empty box, a pose or a grow that is not finite;
    bit 1: no hull with an inside; a flagged row's lines give the weight 0 everywhere)."""
    if poses.dim() != 3:
        raise ValueError('poses must be f32 [n, K, 2], got %s' % (tuple(poses.shape),))
    n, K = int(poses.shape[0]), int(poses.shape[1])
    if n < 1 or n > 65535 or not 1 <= K <= WARP_MAX_POINTS:
        raise ValueError('hull_fit serves 1..65535 rows of 1 <= K <= %d landmarks, got n = %d, K = %d' % (WARP_MAX_POINTS, n, K))
    _check_tensors([('poses', poses, torch.float32, (n, K, 2)), ('boxes', boxes, torch.int32, (n, 5)), ('grow', grow, torch.float32, (n,)),
                    ('edges', edges, torch.float32, (n, K, 3)), ('flags', flags, torch.int32, (n,))])
    call('imm_hull_fit', _p(poses), _p(boxes), _p(grow), K, n, _p(edges), _p(flags), _s())


def morph_hull_u8(src, dst, offsets, hw, donor, donor_offsets, donor_hw, boxes, donor_boxes, links, inv_ramp, texture, ctrl, coef_a, coef_b,
                  gain, edges, inv_soft, max_box_pixels):
    """morph_u8 (gain None) or morph_colour_u8 (gain f32 [n, 3, 2]) with the landmark-hull mask (include/imm_hull.h:
    imm_morph_hull_u8): edges f32 [n, K, 3] (hull_fit's output for these rows) and inv_soft f32 [n] give every pixel of a row's box the
    weight w = clamp(min_k((ny rr + nx cc) + d) * inv_soft, 0, 1); a pixel with w = 0 is left alone, every other is blended with the edge
    ramp times w.  Every other argument as morph_u8 takes it."""
    morph_paste(src, dst, offsets, hw, donor, donor_offsets, donor_hw, boxes, donor_boxes, links, inv_ramp, texture, ctrl, coef_a, coef_b,
                max_box_pixels, gain=gain, **_need('morph_hull_u8', edges=edges, inv_soft=inv_soft))


SEAM_MIN_RING, SEAM_MAX_RING = 16, 256     # ring samples of a row (include/imm_seam.h)


def _check_seam(ring, diff, n, name):
    if ring.dim() != 3 or not SEAM_MIN_RING <= int(ring.shape[1]) <= SEAM_MAX_RING:
        raise ValueError('%s: ring must be f32 [n, B, 2] with %d <= B <= %d, got %s' % (name, SEAM_MIN_RING, SEAM_MAX_RING, tuple(ring.shape)))
    B = int(ring.shape[1])
    _check_tensors([('ring', ring, torch.float32, (n, B, 2)), ('diff', diff, torch.float32, (n, B, 3))])
    return B


def seam_fit(poses, boxes, grow, edges, hull_flags, dirs, src, offsets, hw, donor, donor_offsets, donor_hw, donor_boxes, texture, ctrl,
             coef_a, coef_b, gain, ring, diff, flags):
    """The ring of a seamless morph (include/imm_seam.h: imm_seam_fit): per row B samples of the outline of its grown hull cut with its
    box, ring f32 [n, B, 2] in box-relative pixels, where the rays from the landmarks' centroid along dirs f64 [B, 2] leave it, and at
    every sample the own photo's value minus the morph's mix there, diff f32 [n, B, 3]; flags i32 [n] (bit 0: the hull is flagged or
    the centroid is not strictly inside the region; bit 1: a ray without a positive finite length; a flagged row gets diff = 0 and
    its centroid as every sample).  poses, boxes, grow, edges, hull_flags: hull_fit's inputs and outputs for these rows; the rest as
    morph_hull_u8 takes it (gain None or f32 [n, 3, 2])."""
    if poses.dim() != 3 or ctrl.dim() != 3:
        raise ValueError('poses must be f32 [n, K, 2] and ctrl f32 [n, M, 2], got %s and %s' % (tuple(poses.shape), tuple(ctrl.shape)))
    n, K, M = int(poses.shape[0]), int(poses.shape[1]), int(ctrl.shape[1])
    if n < 1 or n > 65535 or not 1 <= K <= WARP_MAX_POINTS or not 3 <= M <= WARP_MAX_POINTS:
        raise ValueError('seam_fit serves 1..65535 rows of 1 <= K <= %d landmarks and 3 <= M <= %d control points, got n = %d, K = %d, M = %d'
                         % (WARP_MAX_POINTS, WARP_MAX_POINTS, n, K, M))
    B = _check_seam(ring, diff, n, 'seam_fit')
    _check_photos(src, offsets, hw, donor, donor_offsets, donor_hw)
    _check_tensors([('poses', poses, torch.float32, (n, K, 2)), ('boxes', boxes, torch.int32, (n, 5)), ('grow', grow, torch.float32, (n,)),
                    ('edges', edges, torch.float32, (n, K, 3)), ('hull_flags', hull_flags, torch.int32, (n,)),
                    ('dirs', dirs, torch.float64, (B, 2)), ('donor_boxes', donor_boxes, torch.int32, (n, 5)),
                    ('texture', texture, torch.float32, (n,)), ('ctrl', ctrl, torch.float32, (n, M, 2)),
                    ('coef_a', coef_a, torch.float32, (n, M + 3, 2)), ('coef_b', coef_b, torch.float32, (n, M + 3, 2)),
                    ('flags', flags, torch.int32, (n,))])
    if gain is not None:
        _check_tensors([('gain', gain, torch.float32, (n, 3, 2))])
    call('imm_seam_fit', _p(poses), _p(boxes), _p(grow), _p(edges), _p(hull_flags), _p(dirs), _p(src), _p(offsets), _p(hw), int(hw.shape[0]),
         _p(donor), _p(donor_offsets), _p(donor_hw), int(donor_hw.shape[0]), _p(donor_boxes), _p(texture), _p(ctrl), _p(coef_a), _p(coef_b),
         None if gain is None else _p(gain), K, M, B, n, _p(ring), _p(diff), _p(flags), _s())


def morph_seam_u8(src, dst, offsets, hw, donor, donor_offsets, donor_hw, boxes, donor_boxes, links, inv_ramp, texture, ctrl, coef_a, coef_b,
                  gain, edges, inv_soft, ring, diff, seamless, max_box_pixels):
    """morph_hull_u8 with the mean-value membrane (include/imm_seam.h: imm_morph_seam_u8): ring f32 [n, B, 2] and diff f32 [n, B, 3]
    (seam_fit's output for these rows) give every pixel with a weight the correction r, the mean of the row's diffs weighed by the
    pixel's mean-value coordinates in the ring, and the mix takes seamless[b] * r (seamless f32 [n]) in front of the blend.  Every other
    argument as morph_hull_u8 takes it."""
    morph_paste(src, dst, offsets, hw, donor, donor_offsets, donor_hw, boxes, donor_boxes, links, inv_ramp, texture, ctrl, coef_a, coef_b,
                max_box_pixels, gain=gain,
                **_need('morph_seam_u8', edges=edges, inv_soft=inv_soft, ring=ring, diff=diff, seamless=seamless))


CLIP_MAX_WIDTH = 768          # values of a row imm_clip_ema filters: 3 * SEAM_MAX_RING


def clip_rows(boxes, track_flags, mu, points, image_size, feather, mask_feather, own, inv_ramp, inv_soft):
    """One frame's rows of a clip morph (include/imm_clip.h: imm_clip_rows): boxes i32 [F, 5] (the rows this frame was cut with),
    track_flags i32 [F] (track_step's flags of the frame), mu f32 [F, K, 2] and points f32 [F, K, 2] or None (track_step's points or
    points_smooth), feather (a float in [0, 0.5]) and mask_feather f32 [F] or None -> own f32 [F, K, 2] (the landmarks in the frame of
    the box: mu's bits without points, NaN for a lost face), inv_ramp f32 [F, 2] (generation.compose_inv_ramp's bits) and inv_soft f32
    [F] (morphing.hull_inv_soft's bits; None exactly when mask_feather is)."""
    if mu.dim() != 3 or mu.shape[2] != 2:
        raise ValueError('mu must be f32 [F, K, 2], got %s' % (tuple(mu.shape),))
    F, K = int(mu.shape[0]), int(mu.shape[1])
    if F < 1 or F > 65535 or K < 1 or K > WARP_MAX_POINTS:
        raise ValueError('clip_rows serves 1..65535 faces of 1..%d landmarks, got F = %d, K = %d' % (WARP_MAX_POINTS, F, K))
    if (mask_feather is None) != (inv_soft is None):
        raise ValueError('inv_soft is given exactly when mask_feather is')
    specs = [('boxes', boxes, torch.int32, (F, 5)), ('track_flags', track_flags, torch.int32, (F,)), ('mu', mu, torch.float32, (F, K, 2)),
             ('own', own, torch.float32, (F, K, 2)), ('inv_ramp', inv_ramp, torch.float32, (F, 2))]
    if points is not None:
        specs.append(('points', points, torch.float32, (F, K, 2)))
    if mask_feather is not None:
        specs += [('mask_feather', mask_feather, torch.float32, (F,)), ('inv_soft', inv_soft, torch.float32, (F,))]
    _check_tensors(specs)
    for name, t in (('mu', mu), ('points', points)):
        if t is not None and _overlap(t, own):
            raise ValueError('%s overlaps own: the output is written while the inputs are read' % name)
    feather, S = float(feather), int(image_size)
    if not 0.0 <= feather <= 0.5:
        raise ValueError('feather must lie in [0, 0.5], got %r' % (feather,))
    if not 0 < S <= 8192:
        raise ValueError('image_size must lie in (0, 8192], got %r' % (image_size,))
    call('imm_clip_rows', _p(boxes), _p(track_flags), _p(mu), None if points is None else _p(points), K, S, F, feather,
         None if mask_feather is None else _p(mask_feather), _p(own), _p(inv_ramp), None if inv_soft is None else _p(inv_soft), _s())


def clip_ema(x, state, seen, skip, lost, alpha):
    """The filter of a clip morph (include/imm_clip.h: imm_clip_ema): x f32 [n, width] is filtered in place against state f32 [n, width],
    state = state + alpha * (x - state), the first value a row sees (seen i32 [n] == 0) passing through; a row with skip i32 [n] != 0 or
    bit 0 of lost i32 [n] (or None) set leaves its x, state and seen alone.  alpha in (0, 1]."""
    if x.dim() != 2:
        raise ValueError('x must be f32 [n, width], got %s' % (tuple(x.shape),))
    n, width = int(x.shape[0]), int(x.shape[1])
    if n < 1 or n > 65535 or width < 1 or width > CLIP_MAX_WIDTH:
        raise ValueError('clip_ema serves 1..65535 rows of 1..%d values, got n = %d, width = %d' % (CLIP_MAX_WIDTH, n, width))
    specs = [('x', x, torch.float32, (n, width)), ('state', state, torch.float32, (n, width)), ('seen', seen, torch.int32, (n,)),
             ('skip', skip, torch.int32, (n,))]
    if lost is not None:
        specs.append(('lost', lost, torch.int32, (n,)))
    _check_tensors(specs)
    if _overlap(x, state):
        raise ValueError('x overlaps state')
    alpha = float(alpha)
    if not 0.0 < alpha <= 1.0:
        raise ValueError('alpha must lie in (0, 1], got %r' % (alpha,))
    call('imm_clip_ema', _p(x), _p(state), _p(seen), _p(skip), None if lost is None else _p(lost), n, width, alpha, _s())


REDACT_MAX_BLOCKS = 64        # cells along the longer side of a redacted box (include/imm_redact.h)
REDACT_MODES = {'pixelate': 0, 'smooth': 1}      # IMM_REDACT_*


def _check_redact(name, buf, offsets, hw, boxes, blocks, cells):
    """What the two redaction entries share: the packed buffer, the box rows, blocks and the cells buffer -> (n, blocks)."""
    if boxes.dim() != 2:
        raise ValueError('boxes must be int32 [n, 5], got %s' % (tuple(boxes.shape),))
    n = int(boxes.shape[0])
    if n < 1 or n > 65535:
        raise ValueError('%s serves 1..65535 rows, got n = %d' % (name, n))
    if isinstance(blocks, bool) or int(blocks) != blocks or not 1 <= int(blocks) <= REDACT_MAX_BLOCKS:
        raise ValueError('blocks must be an int in [1, %d], got %r' % (REDACT_MAX_BLOCKS, blocks))
    blocks = int(blocks)
    _check_tensors([('photos', buf, torch.uint8, (None,)), ('hw', hw, torch.int32, (None, 2))])
    if hw.shape[0] < 1:
        raise ValueError('hw must hold at least one image, got %s' % (tuple(hw.shape),))
    _check_tensors([('boxes', boxes, torch.int32, (n, 5)), ('offsets', offsets, torch.int64, (hw.shape[0],)),
                    ('cells', cells, torch.uint8, (n, blocks * blocks * 3))])
    if _overlap(cells, buf):
        raise ValueError('cells overlaps the photos')
    return n, blocks


def redact_cells_u8(src, offsets, hw, boxes, blocks, cells):
    """The cell means of every row's box (include/imm_redact.h: imm_redact_cells_u8): src u8 [bytes] with offsets i64 [images] and hw i32
    [images, 2] (a packed buffer, as warp_u8 reads it) and boxes i32 [n, 5] -> cells u8 [n, blocks * blocks * 3]: per row the box cut
    into gy x gx square cells of side ceil(max(H, W) / blocks), every cell the mean (half up, in integers) of the bytes it covers inside
    the photo, dense as [gy, gx, 3] at the start of the row's slice; every other byte, and the slice of a row that is not active, 0."""
    n, blocks = _check_redact('redact_cells_u8', src, offsets, hw, boxes, blocks, cells)
    call('imm_redact_cells_u8', _p(src), _p(offsets), _p(hw), int(hw.shape[0]), _p(boxes), blocks, n, _p(cells), _s())


def redact_u8(dst, offsets, hw, boxes, links, inv_ramp, cells, blocks, mode, max_box_pixels, edges=None, inv_soft=None, hull_flags=None):
    """The packed u8 photos dst redacted in place (include/imm_redact.h: imm_redact_u8): every pixel of row b's box takes its cell's mean
    (mode 0 or 'pixelate') or the bilinear sample of the grid of means (1 or 'smooth') from cells u8 [n, blocks * blocks * 3]
    (redact_cells_u8's output for these rows, taken from the ORIGINAL pixels), blended with the edge ramp inv_ramp f32 [n, 2] and rounded
    to u8, in row order.  boxes, links, max_box_pixels as warp_u8 takes them.  edges f32 [n, K, 3], inv_soft f32 [n] and hull_flags i32
    [n] (hull_fit's output for these rows) come together or not at all: with them the ramp is multiplied by the hull's weight, a pixel
    outside the hull is left alone, and a row whose flag is not 0 is redacted over its WHOLE box."""
    n, blocks = _check_redact('redact_u8', dst, offsets, hw, boxes, blocks, cells)
    mode = REDACT_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if isinstance(mode, bool) or mode not in (0, 1):
        raise ValueError("mode must be 0 ('pixelate') or 1 ('smooth'), got %r" % (mode,))
    _check_tensors([('links', links, torch.int32, (n, 2)), ('inv_ramp', inv_ramp, torch.float32, (n, 2))])
    if int(max_box_pixels) < 1:
        raise ValueError('max_box_pixels must be positive, got %r' % (max_box_pixels,))
    trio = dict(edges=edges, inv_soft=inv_soft, hull_flags=hull_flags)
    absent = [k for k, t in trio.items() if t is None]
    if absent and len(absent) < 3:
        raise ValueError('edges, inv_soft and hull_flags come together: %s is None' % absent[0])
    K = 0
    if edges is not None:
        if edges.dim() != 3 or not 1 <= int(edges.shape[1]) <= WARP_MAX_POINTS:
            raise ValueError('edges must be f32 [n, K, 3] with 1 <= K <= %d, got %s' % (WARP_MAX_POINTS, tuple(edges.shape)))
        K = int(edges.shape[1])
        _check_tensors([('edges', edges, torch.float32, (n, K, 3)), ('inv_soft', inv_soft, torch.float32, (n,)),
                        ('hull_flags', hull_flags, torch.int32, (n,))])
    for k, t in dict(trio, links=links, inv_ramp=inv_ramp, boxes=boxes, offsets=offsets, hw=hw).items():
        if t is not None and _overlap(t, dst):
            raise ValueError('%s overlaps dst' % k)
    call('imm_redact_u8', _p(dst), _p(offsets), _p(hw), int(hw.shape[0]), _p(boxes), _p(links), _p(inv_ramp), _p(cells), blocks, int(mode),
         None if edges is None else _p(edges), None if edges is None else _p(inv_soft), None if edges is None else _p(hull_flags), K, n,
         int(max_box_pixels), _s())


ANNOTATE_BITS = {'points': 1, 'box': 2, 'hull': 4, 'label': 8}      # IMM_ANNOTATE_*
ANNOTATE_MAX_GROUPS, ANNOTATE_MAX_PAD = 16, 64                      # include/imm_annotate.h


def annotate_points(mu, boxes, points):
    """Landmarks from the frame of their box to photo pixels (include/imm_annotate.h: imm_annotate_points): mu f32 [n, K, 2] in [-1, 1]
    of boxes i32 [n, 5] -> points f32 [n, K, 2], py = y0 + (mu_y + 1) * (0.5 * H) in f64 rounded once; a value that is not finite is
    stored as it is."""
    if mu.dim() != 3 or mu.shape[2] != 2:
        raise ValueError('mu must be f32 [n, K, 2], got %s' % (tuple(mu.shape),))
    n, K = int(mu.shape[0]), int(mu.shape[1])
    if n < 1 or n > 65535 or K < 1 or K > WARP_MAX_POINTS:
        raise ValueError('annotate_points serves 1..65535 rows of 1..%d landmarks, got n = %d, K = %d' % (WARP_MAX_POINTS, n, K))
    _check_tensors([('mu', mu, torch.float32, (n, K, 2)), ('boxes', boxes, torch.int32, (n, 5)), ('points', points, torch.float32, (n, K, 2))])
    if _overlap(mu, points):
        raise ValueError('mu overlaps points: the output is written while the input is read')
    call('imm_annotate_points', _p(mu), _p(boxes), K, n, _p(points), _s())


def annotate_u8(dst, offsets, hw, boxes, links, palette, draw_bits, thickness, pad, label_scale, max_box_pixels, marks=None, group_style=None,
                mark_style=None, edges=None, status=None, labels=None):
    """The packed u8 photos dst drawn into in place (include/imm_annotate.h: imm_annotate_u8).  boxes, links, max_box_pixels as warp_u8
    takes them (max_box_pixels: the largest extent, a box grown by pad on every side); palette u8 [P, 3]; draw_bits a sum of
    ANNOTATE_BITS.  With 'points': marks f32 [G, n, K, 2] in photo pixels (group G - 1 the markers, the groups before it the trail, oldest
    first), group_style f32 [G, 4] = (R, 1 / (2 R), h, alpha) and mark_style u8 [K, 4] = (r, g, b, shape).  With 'hull': edges f32
    [n, K, 3] (hull_fit's lines).  With 'label': labels i32 [n].  status i32 [n] or None picks every row's colour; a row with bit 0 set
    draws its frame and label only."""
    if boxes.dim() != 2:
        raise ValueError('boxes must be int32 [n, 5], got %s' % (tuple(boxes.shape),))
    n = int(boxes.shape[0])
    if n < 1 or n > 65535:
        raise ValueError('annotate_u8 serves 1..65535 rows, got n = %d' % n)
    for name, v, lo, hi in (('draw_bits', draw_bits, 0, 15), ('thickness', thickness, 1, 16), ('pad', pad, 0, ANNOTATE_MAX_PAD),
                            ('label_scale', label_scale, 1, 8), ('max_box_pixels', max_box_pixels, 1, 2 ** 31 - 1)):
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
            raise ValueError('%s must be an int in [%d, %d], got %r' % (name, lo, hi, v))
    bits = int(draw_bits)
    _check_tensors([('photos', dst, torch.uint8, (None,)), ('hw', hw, torch.int32, (None, 2)), ('palette', palette, torch.uint8, (None, 3))])
    if hw.shape[0] < 1 or not 1 <= int(palette.shape[0]) <= 32:
        raise ValueError('hw must hold at least one image and palette 1..32 colours, got %s and %s' % (tuple(hw.shape), tuple(palette.shape)))
    _check_tensors([('boxes', boxes, torch.int32, (n, 5)), ('offsets', offsets, torch.int64, (hw.shape[0],)), ('links', links, torch.int32, (n, 2))])
    given = dict(boxes=boxes, offsets=offsets, hw=hw, links=links, palette=palette)
    K = G = 1
    if bits & 1:
        _need('annotate_u8 with points', marks=marks, group_style=group_style, mark_style=mark_style)
        if marks.dim() != 4 or not 1 <= int(marks.shape[0]) <= ANNOTATE_MAX_GROUPS or not 1 <= int(marks.shape[2]) <= WARP_MAX_POINTS:
            raise ValueError('marks must be f32 [G, n, K, 2] with 1 <= G <= %d and 1 <= K <= %d, got %s'
                             % (ANNOTATE_MAX_GROUPS, WARP_MAX_POINTS, tuple(marks.shape)))
        G, K = int(marks.shape[0]), int(marks.shape[2])
        _check_tensors([('marks', marks, torch.float32, (G, n, K, 2)), ('group_style', group_style, torch.float32, (G, 4)),
                        ('mark_style', mark_style, torch.uint8, (K, 4))])
        given.update(marks=marks, group_style=group_style, mark_style=mark_style)
    if bits & 4:
        _need('annotate_u8 with the hull', edges=edges)
        if edges.dim() != 3 or not 1 <= int(edges.shape[1]) <= WARP_MAX_POINTS or (bits & 1 and int(edges.shape[1]) != K):
            raise ValueError('edges must be f32 [n, K, 3] with 1 <= K <= %d (the K of marks), got %s' % (WARP_MAX_POINTS, tuple(edges.shape)))
        K = int(edges.shape[1])
        _check_tensors([('edges', edges, torch.float32, (n, K, 3))])
        given.update(edges=edges)
    if bits & 8:
        _need('annotate_u8 with labels', labels=labels)
        _check_tensors([('labels', labels, torch.int32, (n,))])
        given.update(labels=labels)
    if status is not None:
        _check_tensors([('status', status, torch.int32, (n,))])
        given.update(status=status)
    for k, t in given.items():
        if _overlap(t, dst):
            raise ValueError('%s overlaps dst' % k)
    opt = lambda t, bit: _p(t) if bits & bit else None
    call('imm_annotate_u8', _p(dst), _p(offsets), _p(hw), int(hw.shape[0]), _p(boxes), _p(links), opt(marks, 1), opt(group_style, 1),
         opt(mark_style, 1), opt(edges, 4), None if status is None else _p(status), _p(palette), int(palette.shape[0]), opt(labels, 8), bits,
         int(thickness), int(pad), int(label_scale), K, G, n, int(max_box_pixels), _s())


def masked_sse_pool(a, b, batch, s, c, mask, S, partial, pool_a, pool_b):
    call('imm_masked_sse_pool', _p(a), _p(b), dtype_enum(a.dtype), batch, s, c, _p(mask), S, _p(partial), _p(pool_a), _p(pool_b), _s())


def unpool_tap_grad(da, dpool, a_pred, a_gt, batch, s, c, mask, S, coef, idx):
    call('imm_unpool_tap_grad', _p(da), _p(dpool), _p(a_pred), _p(a_gt), dtype_enum(da.dtype), batch, s, c, _p(mask), S,
         _p(coef), idx, _s())


class ConvGroup(object):
    """Descriptor array + filter pointer array for imm_conv2d_group (kept alive by this object)."""

    def __init__(self, descs, wts):
        assert 1 <= len(descs) <= 4 and len(descs) == len(wts)
        self.n = len(descs)
        self.descs = (ConvDesc * self.n)(*descs)
        self.wts = wts
        self.ptrs = (C.c_void_p * self.n)(*[w.data_ptr() for w in wts])


def conv2d_group(group, x, y, stats=None, mask=None):
    call('imm_conv2d_group', C.cast(group.descs, C.c_void_p), group.n, dtype_enum(x.dtype), _p(x), C.cast(group.ptrs, C.c_void_p),
         _p(y), _p(stats), _p(mask), _s())


def conv_first_supported(batch, s, co, ldy):
    return bool(L.load().imm_conv_first_supported(batch, s, co, ldy))


def conv_first_stats_blocks(batch, s):
    n = L.load().imm_conv_first_stats_blocks(batch, s)
    if n <= 0:
        raise L.ImmHipError('imm_conv_first_stats_blocks(%d, %d)' % (batch, s))
    return n


def conv_first(image, wt, bias, y, ldy, stats, batch, s, co, flags):
    """First encoder convolution (7x7 over RGB) straight from the f32 image (imm_conv_first); wt = the 7x1 packed filter image."""
    call('imm_conv_first', _p(image), _p(wt), int(wt.shape[1]), _p(bias), _p(y), ldy, _p(stats), dtype_enum(y.dtype), batch, s, co,
         flags, _s())


def conv2d_dgrad_s2_supported(batch, h, w, lddy, c_dx, lddx):
    """dy [batch,h,w] with pixel stride lddy -> dx [batch,2h,2w,c_dx]: served by the one-launch four-class kernel?"""
    return bool(L.load().imm_conv2d_dgrad_s2_supported(batch, h, w, lddy, c_dx, lddx))


def conv2d_dgrad_s2(dy, lddy, wt, dx, lddx, c_dx, batch, h, w):
    """Data gradient of a 3x3 stride-2 SAME convolution as ONE launch (imm_conv2d_dgrad_s2): wt = the mode-1 packed image
    [rows >= c_dx][9 * lddy]."""
    call('imm_conv2d_dgrad_s2', _p(dy), lddy, _p(wt), int(wt.shape[1]), _p(dx), lddx, c_dx, dtype_enum(dy.dtype), batch, h, w, _s())


def conv2d_group_stats_blocks(group):
    n = L.load().imm_conv2d_group_stats_blocks(C.cast(group.descs, C.c_void_p), group.n)
    if n <= 0:
        raise L.ImmHipError('imm_conv2d_group_stats_blocks: ' + L.load().imm_last_error().decode())
    return n


# ---- RCCL through the C-ABI (imm_rccl_*): the data-parallel gradient exchange without torch.distributed in the loop ----------
class RcclComm:
    """Communicator for the current device.  The 128-byte unique id is made by rank 0 and exchanged over the (already
    initialised) torch.distributed process group, used here as the host-side side channel only."""

    def __init__(self, rank, world, group=None):
        import torch.distributed as dist
        uid = torch.zeros(128, dtype=torch.uint8)
        if rank == 0:
            buf = (C.c_ubyte * 128)()
            call('imm_rccl_unique_id', C.cast(buf, C.c_void_p))
            uid = torch.tensor(list(buf), dtype=torch.uint8)
        if world > 1:
            obj = [uid]
            # `rank` is the rank inside `group`; broadcast's src is a GLOBAL rank
            src = dist.get_global_rank(group, 0) if group is not None else 0
            dist.broadcast_object_list(obj, src=src, group=group)
            uid = obj[0]
        self._uid = (C.c_ubyte * 128)(*[int(x) for x in uid])
        self._comm = C.c_void_p()
        call('imm_rccl_init', rank, world, C.cast(self._uid, C.c_void_p), C.byref(self._comm))
        self.world = world

    def all_reduce_sum(self, flat_f32):
        """In-place sum over ranks, enqueued on torch's current stream (capturable into a HIP graph)."""
        assert flat_f32.dtype == torch.float32 and flat_f32.is_contiguous()
        call('imm_rccl_allreduce', self._comm, _p(flat_f32), flat_f32.numel(), _s())

    def destroy(self):
        if self._comm:
            call('imm_rccl_destroy', self._comm)
            self._comm = C.c_void_p()
