"""Exact-arithmetic kernel tests: integer data, compared bit for bit, on a real MI355X.

The tolerance tests (tests/test_kernels_gpu.py) feed randn and accept 1e-2 relative plus 2e-3 of the tensor's maximum for bf16:
more than one bf16 ulp, so truncation instead of round-to-nearest-even, ties rounded away, an accumulator parked in 16 bits, a
batch-norm sum taken from the rounded value, or one small lost term all pass them.  Here every operand is a small integer (a bias a
half-integer): every product and every partial sum, in any order, is exact in f32 (tests/exact_data.py), so a 16-bit output must
equal RNE16(exact) bit for bit, and an f32 output, a filter gradient and the f64 total of the batch-norm partial rows must equal
the exact value.  Zero tolerance; every case asserts the (family, variant) key of the kernel it is named after; every output sits
in a guarded buffer (tests/guarded.py).  tests/test_exact_cpu.py shows, without a GPU, that every case meets the premise and that
its 16-bit outputs do round (>= 20 % not representable, >= 5 % ties, >= 5 % inexact non-ties), and that in every batch-norm-sum run
the sums of the rounded outputs differ from the exact sums.

Triage of a failure: exact_equal says whether the stored value is the truncated or the ties-away rounding of the exact one.  If the
forms without a 16-bit rounding (f32 heads, filter gradients) are exact for a family and only its 16-bit store differs, the store
is at fault; if neither, a term is lost or doubled.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded                                                              # noqa: E402
from guarded import untouched                                               # noqa: E402
import exact_data as E                                                      # noqa: E402
from exact_data import exact_equal, rne16                                   # noqa: E402
from test_kernels_gpu import CONV_FAMILY, CONV_VARIANT, DEV, check_family, dev, padded, run_conv   # noqa: E402

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize('dt', E.DTYPES, ids=E.DT_IDS)


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


def stored(y, v, dt, what):
    """y (a kernel output of exact value v): the exact value itself when y is f32, else its one RNE to dt."""
    if y.dtype == torch.float32:
        exact_equal(y, v, what)
    else:
        exact_equal(y, rne16(v, dt), what, exact=v)


def totals(stats, s1, s2, what):
    """The partial rows [nblk][2][co], summed in f64 on the host, are (s1, s2) exactly: every row is an exact f32 value."""
    s = stats.double().sum(0).cpu()
    exact_equal(s[0], s1, what + ': sum v')
    exact_equal(s[1], s2, what + ': second sum')


# ----------------------------------------------------------------------------------------------
# a. forward: one case per family and variant of imm_conv2d, five epilogues each
# ----------------------------------------------------------------------------------------------
def test_forward_table_names_the_suites_own_families():
    for tag, (fam, key) in E.FWD_KEY.items():
        assert fam == CONV_FAMILY.get(tag, 's2f' if tag in ('one_nblk_two_slices', 'enc_conv5_64to128') else 'igemm'), tag
        assert CONV_VARIANT.get(tag, key) == key, tag


@DT
@pytest.mark.parametrize('tag', E.FWD_TAGS)
def test_conv_forward_exact(ops, tag, dt):
    """1 bias, 2 bias + ReLU, 3 bias + mask at high amplitude (the store rounds); 4 bias + batch-norm sums, 5 bias + mask + the
    batch-norm backward sums at low amplitude plus a few spikes that the store rounds (exact_data.LOW_SPIKE: without them a kernel
    that summed what it stored would pass).  The sums are those of the UNROUNDED f32 value v after bias, ReLU and mask."""
    from imm_amd import _lib as L
    _B, _H, _ci_real, ci_pad, co, k, stride, out_f32 = E.fwd_shapes()[tag]

    def run(name, e, flags, mask=None):
        key = E.fwd_key(tag, name)
        args = (ops, e.x.to(dt), e.w.float(), e.bias.float(), k, stride, co, ci_pad, out_f32)
        if key is None:                                     # declined by the entry point, not silently served by something else
            with pytest.raises(L.ImmHipError):
                run_conv(*args, extra_flags=flags, mask=mask)
            return None, None
        y, stats, desc = run_conv(*args, extra_flags=flags, mask=mask)
        assert ops.conv2d_variant(desc, dt) == key, (tag, name, ops.conv2d_variant(desc, dt), key)
        if name == 'bias' and key[0] != 's2f':              # (the suite's CONV_FAMILY has no entry for the stride-2 forward tags)
            check_family(ops, desc, dt, tag)
        assert untouched(y[..., co:]), 'padding channels [co, ldy) belong to the caller: imm_conv2d must not write them'
        return y[..., :co], stats

    e = E.fwd_data(tag, dt, low=False)
    y, _ = run('bias', e, 0)
    stored(y, e.y, dt, '%s/bias' % tag)
    y, _ = run('relu', e, L.CONV_RELU)
    stored(y, e.y.clamp(min=0), dt, '%s/relu' % tag)
    md = dev(e.mask.to(dt))
    y, _ = run('mask', e, L.CONV_MASK, md)
    if y is not None:
        stored(y, torch.where(e.mask > 0, e.y, 0.), dt, '%s/mask' % tag)
        assert bool((y.cpu()[e.mask <= 0].view(torch.int16) == 0).all()), 'mask_ref <= 0 must store +0'

    lo = E.fwd_data(tag, dt, low=True)
    y, stats = run('stats', lo, L.CONV_STATS)
    stored(y, lo.y, dt, '%s/stats y' % tag)
    totals(stats, lo.y.sum((0, 1, 2)), (lo.y * lo.y).sum((0, 1, 2)), '%s/stats' % tag)
    y, stats = run('stats_mask', lo, L.CONV_STATS | L.CONV_MASK, dev(lo.mask.to(dt)))
    if y is not None:
        v = torch.where(lo.mask > 0, lo.y, 0.)
        stored(y, v, dt, '%s/stats+mask y' % tag)
        totals(stats, v.sum((0, 1, 2)), (v * lo.mask).sum((0, 1, 2)), '%s/stats+mask' % tag)


@DT
@pytest.mark.parametrize('B,S,co', E.FIRST_CASES, ids=['128px_co32', '32px_co20'])
def test_first_conv_from_the_f32_image_exact(ops, B, S, co, dt):
    """imm_conv_first from integer pixels: bias, bias + ReLU, bias + batch-norm sums; it has no mask and must refuse one."""
    from imm_amd import _lib as L
    ldy = ops.round_up(co, 8)
    assert ops.conv_first_supported(B, S, co, ldy)

    def run(e, flags, with_stats=False):
        wt = guarded.out((128, 224), dt, DEV, fill=0)
        ops.pack_weights(e.w.float().to(DEV).contiguous(), wt, 0, 7, 1, 21, co, 32, 128, 224)
        y = guarded.out((B, S, S, ldy), dt, DEV)
        stats = guarded.out((ops.conv_first_stats_blocks(B, S), 2, co), torch.float32, DEV) if with_stats else None
        ops.conv_first(dev(e.x.float()), wt, e.bias.float().to(DEV), y, ldy, stats, B, S, co, L.CONV_BIAS | flags)
        torch.cuda.synchronize()
        assert untouched(y[..., co:])
        return y[..., :co], stats

    e = E.first_data(B, S, co, dt, low=False)
    y, _ = run(e, 0)
    stored(y, e.y, dt, 'conv_first/bias')
    y, _ = run(e, L.CONV_RELU)
    stored(y, e.y.clamp(min=0), dt, 'conv_first/relu')
    lo = E.first_data(B, S, co, dt, low=True)
    y, stats = run(lo, L.CONV_STATS, True)
    stored(y, lo.y, dt, 'conv_first/stats y')
    totals(stats, lo.y.sum((0, 1, 2)), (lo.y * lo.y).sum((0, 1, 2)), 'conv_first/stats')
    with pytest.raises(L.ImmHipError):
        run(lo, L.CONV_MASK)


# ----------------------------------------------------------------------------------------------
# b. data gradient
# ----------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize('tag', list(E.DGRAD))
def test_conv_dgrad_exact(ops, tag, dt):
    (B, H, ci_real, ci_pad, co, co_pad, k, stride), key, amps = E.DGRAD[tag]
    e = E.dgrad_data('dgrad', tag, (B, H, ci_real, co, k, stride), dt, amps)
    desc = ops.dgrad_desc(B, H, H, ci_real, ci_pad, co_pad, co_pad, k, stride, 0)
    assert ops.conv2d_variant(desc, dt) == key
    check_family(ops, desc, dt, tag)
    rows = ops.round_up(ci_real, 128)
    wt = guarded.out((rows, desc.kpad), dt, DEV, fill=0)
    ops.pack_weights(e.w.float().to(DEV).contiguous(), wt, 1, k, k, ci_real, co, co_pad, rows, desc.kpad)
    dx = guarded.out((B, H, H, ci_pad), dt, DEV)
    ops.conv2d(desc, padded(e.dy.to(dt), co_pad), wt, None, dx)
    torch.cuda.synchronize()
    stored(dx[..., :ci_real], e.dx, dt, 'dgrad/' + tag)
    assert untouched(dx[..., ci_real:])


@DT
def test_conv_group_stride2_dgrad_exact(ops, dt):
    """imm_conv2d_group: the four parity classes of a stride-2 data gradient in one launch, scattered into dx."""
    (B, H, ci, co), key, amps = E.GROUP
    e = E.dgrad_data('group', 'group', (B, H, ci, co, 3, 2), dt, amps)
    classes = ops.dgrad_s2_class_descs(B, H, H, ci, ci, co, co, 3)
    assert len(classes) == 4
    rows = ops.round_up(ci, 128)
    wts = []
    for d, mode in classes:
        assert ops.conv2d_variant(d, dt) == key
        wt = guarded.out((rows, d.kpad), dt, DEV, fill=0)
        ops.pack_weights(e.w.float().to(DEV).contiguous(), wt, mode, 3, 3, ci, co, co, rows, d.kpad)
        wts.append(wt)
    got = guarded.out((B, H, H, ci), dt, DEV)
    ops.conv2d_group(ops.ConvGroup([d for d, _m in classes], wts), dev(e.dy.to(dt)), got)
    torch.cuda.synchronize()
    stored(got, e.dx, dt, 'conv2d_group')


@DT
@pytest.mark.parametrize('tag', list(E.S2D))
def test_conv_dgrad_stride2_one_launch_exact(ops, tag, dt):
    """imm_conv2d_dgrad_s2: four accumulator sets over one dy halo (the deep-K form and the filter-in-LDS form)."""
    (B, H, ci, co), amps = E.S2D[tag]
    e = E.dgrad_data('s2d', tag, (B, H, ci, co, 3, 2), dt, amps)
    h = H // 2
    assert ops.conv2d_dgrad_s2_supported(B, h, h, co, ci, ci)
    rows = ops.round_up(ci, 128)
    wt = guarded.out((rows, 9 * co), dt, DEV, fill=0)
    ops.pack_weights(e.w.float().to(DEV).contiguous(), wt, 1, 3, 3, ci, co, co, rows, 9 * co)
    dx = guarded.out((B, H, H, ci), dt, DEV)
    ops.conv2d_dgrad_s2(dev(e.dy.to(dt)), co, wt, dx, ci, ci, B, h, h)
    torch.cuda.synchronize()
    stored(dx, e.dx, dt, 'dgrad_s2/' + tag)


@DT
@pytest.mark.parametrize('tag', list(E.TAP))
def test_conv_dgrad_with_tap_epilogue_exact(ops, tag, dt):
    """imm_conv2d_tap = [a_pred > 0] * (round16(conv) + coef * loss_mask * (a_pred - a_gt)), rounded once more: the inner rounding
    is part of the ABI (it is what makes the fused form equal the two launches), and only an exact conv can show where it sits."""
    (B, H, cin, cout, l1), amps = E.TAP[tag]
    S = 128
    e = E.dgrad_data('tap', tag, (B, H, cin, cout, 3, 1), dt, amps)
    a_gt, a_pred = E.ints((B, H, H, cin), 4, 173), E.ints((B, H, H, cin), 4, 174)
    lmask = E.ints((B, S, S), 3, 175, lo=0)
    coef = 0.5
    desc = ops.dgrad_desc(B, H, H, cin, cin, cout, cout, 3, 1, 0)
    assert ops.conv2d_tap_supported(desc) and ops.conv2d_variant(desc, dt) == E.TAP_KEY
    wt = guarded.out((ops.round_up(cin, 128), desc.kpad), dt, DEV, fill=0)
    ops.pack_weights(e.w.float().to(DEV).contiguous(), wt, 1, 3, 3, cin, cout, cout, wt.shape[0], desc.kpad)
    dz, apd, agd = dev(e.dy.to(dt)), dev(a_pred.to(dt)), dev(a_gt.to(dt))
    coefd = torch.tensor([0.0, coef, 0.0], device=DEV)
    inner = rne16(e.dx, dt).view(dt).to(torch.float64)
    assert bool((inner != e.dx).any())
    d = a_pred - a_gt
    d = torch.sign(d) if l1 else d
    for mk in (lmask, None):
        got = guarded.out((B, H, H, cin), dt, DEV)
        ops.conv2d_tap(desc, dz, wt, got, apd, agd, cin, None if mk is None else mk.float().to(DEV), S, coefd, 1, l1)
        torch.cuda.synchronize()
        m = 1.0 if mk is None else mk[:, ::S // H, ::S // H].unsqueeze(-1)
        t = torch.where(a_pred > 0, inner + coef * m * d, 0.)
        stored(got, t, dt, 'conv2d_tap/%s/%s' % (tag, 'masked' if mk is not None else 'no mask'))


# ----------------------------------------------------------------------------------------------
# c. filter gradient: f32 out, no rounding anywhere — dw after the reduce IS the exact integer gradient
# ----------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize('tag', list(E.WGRAD))
def test_conv_wgrad_exact(ops, tag, dt):
    """The transpose-read kernel, the generic one, the LDS-halo kernel (3x3, the 7x1 first layer, stride 2) at its own split count,
    and the same 3x3 job at another split count (which the single entry point gives to the transpose-read kernel)."""
    B, H, ci_real, ci_pad, co, lddy, k, kw, stride, nsplit, key = E.WGRAD[tag]
    e = E.wgrad_data(tag, B, H, ci_real, co, k, kw, stride, dt, 5)
    desc = ops.fwd_desc(B, H, H, ci_pad, ci_pad, co, lddy, k, stride, 0, kw=kw)
    assert ops.conv2d_wgrad_variant(desc, lddy, dt)[0] == key
    own = ops.conv2d_wgrad_splits(desc, lddy)             # > 0: the split count at which the LDS-halo kernel takes the job
    ns = nsplit or own
    assert ns > 0 and (nsplit == 0 or nsplit != own), (tag, nsplit, own)
    slab = guarded.out((ns, desc.kpad, co), torch.float32, DEV)
    ops.conv2d_wgrad(desc, padded(e.x.to(dt), ci_pad), padded(e.dy.to(dt), lddy), lddy, slab, ns)
    dw = guarded.out((k, kw, ci_real, co), torch.float32, DEV)
    ops.conv2d_wgrad_reduce(slab, ns, k, kw, ci_pad, ci_real, co, desc.kpad, dw)
    torch.cuda.synchronize()
    exact_equal(dw, e.dw, 'wgrad/' + tag)


@DT
def test_conv_wgrad_multi_exact(ops, dt):
    """imm_conv2d_wgrad_multi on the job list of test_conv_wgrad_multi_equals_single_launches: every job's reduced gradient."""
    made, jobs = [], []
    for i, (B, H, ci, co, lddy, k, stride, nsplit) in enumerate(E.WGRAD_MULTI):
        e = E.wgrad_data('multi%d' % i, B, H, ci, co, k, k, stride, dt, 500 + i)
        desc = ops.fwd_desc(B, H, H, ci, ci, co, lddy, k, stride, 0)
        assert ops.conv2d_wgrad_variant(desc, lddy, dt)[0] == E.WGRAD_MULTI_KEYS[i], i
        slab = guarded.out((nsplit, desc.kpad, co), torch.float32, DEV)
        jobs.append((desc, dev(e.x.to(dt)), padded(e.dy.to(dt), lddy), lddy, slab, nsplit))
        made.append((desc, slab, nsplit, k, ci, co, e))
    ops.conv2d_wgrad_multi(ops.WgradMulti(jobs, dt))
    torch.cuda.synchronize()
    for i, (desc, slab, nsplit, k, ci, co, e) in enumerate(made):
        dw = guarded.out((k, k, ci, co), torch.float32, DEV)
        ops.conv2d_wgrad_reduce(slab, nsplit, k, k, ci, ci, co, desc.kpad, dw)
        torch.cuda.synchronize()
        exact_equal(dw, e.dw, 'wgrad_multi/job%d (variant %d)' % (i, E.WGRAD_MULTI_KEYS[i]))


# ----------------------------------------------------------------------------------------------
# d. plain sums that feed the same layers
# ----------------------------------------------------------------------------------------------
@DT
def test_colsum_exact(ops, dt):
    c, npix = E.COLSUM_SHAPE
    x = E.colsum_data(dt)
    part = guarded.out((ops.colsum_blocks(npix, c), c), torch.float32, DEV)
    out = guarded.out((c,), torch.float32, DEV)
    ops.colsum(dev(x.to(dt)), npix, c, c, c, part, out)
    torch.cuda.synchronize()
    exact_equal(out, x.sum(0), 'colsum')


@DT
def test_masked_sse_and_pool_exact(ops, dt):
    """imm_masked_sse (l2 and l1) and imm_masked_sse_pool: the f64 total of the partials is the exact masked sum; the pooled
    halves are the exact maxima."""
    from imm_amd import _lib as L
    B, s, c, S = E.SSE_SHAPE
    a, b, mask = E.sse_data(dt)
    ad, bd, md = dev(a.to(dt)), dev(b.to(dt)), dev(mask.float())
    m4 = mask[:, ::S // s, ::S // s].unsqueeze(-1)
    d = a - b
    for l1, ref in ((False, (m4 * d * d).sum()), (True, (m4 * d.abs()).sum())):
        part = guarded.out((L.SSE_BLOCKS,), torch.float32, DEV)
        ops.masked_sse(ad, bd, B, s, c, md, S, part, l1=l1)
        torch.cuda.synchronize()
        exact_equal(part.double().sum().reshape(1), ref.reshape(1), 'masked_sse l1=%s' % l1)
    part = guarded.out((L.SSE_BLOCKS,), torch.float32, DEV)
    pa, pb = guarded.out((B, s // 2, s // 2, c), dt, DEV), guarded.out((B, s // 2, s // 2, c), dt, DEV)
    ops.masked_sse_pool(ad, bd, B, s, c, md, S, part, pa, pb)
    torch.cuda.synchronize()
    exact_equal(part.double().sum().reshape(1), (m4 * d * d).sum().reshape(1), 'masked_sse_pool')
    for got, src, what in ((pa, a, 'pool_a'), (pb, b, 'pool_b')):
        want = src.reshape(B, s // 2, 2, s // 2, 2, c).amax(dim=(2, 4))
        stored(got, want, dt, 'masked_sse_pool/' + what)
