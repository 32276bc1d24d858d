"""The kernels of imm_amd/csrc/loss_optim.hip on a real MI355X: the error sums, imm_perceptual_finalize, the gradient injection at the
taps and imm_clip_adam_step, in every storage type the kernel dispatches on (bf16, f16, f32).

A. Error sums, exact: integer features, images and masks (a different mask per sample); the f64 host sum of the 512 partials is the
   exact masked sum, l2 and l1, at r = S / s in {1, 2, 4, 8}, one vector per pixel and 17, and on the one shape at which
   sse_f32_thread_sum takes its four-pixel pass (B 7, S 256) for every (lda, ldb) path, the wide columns holding NaN.
B. imm_perceptual_finalize: partial tables whose f64 sum is exact and whose f32 sum is not, bit for bit; every output and the new
   agg against f64 within the bounds of tests/loss_reference.py.
C. Gradient injection, exact: integer activations and gradients, a dyadic coefficient, integer masks; what is stored is the one
   RNE of the exact value, every zero +0; the pooling tie rule is the restatement's (the first maximum), not a second kernel's.
D. The optimizer: one exact step (the prepared gradients, the chunk sums, the norms, m and v bit for bit), the own-tensor scan of
   the default prologue beyond 256 chunks, three steps of Adam / Adadelta / Adagrad on randn data against f64 element-wise,
   the learning rate, the skip rule and imm_weight_decay_loss.

Every bounded test prints its largest err/bound and the share it left out (run with -s).  Every device tensor is a guarded buffer
(tests/guarded.py).  What the data must satisfy for all this to mean anything is asserted without a GPU in tests/test_loss_cpu.py.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded                                                              # noqa: E402
from guarded import untouched                                               # noqa: E402
import exact_data as E                                                      # noqa: E402
import loss_reference as R                                                  # noqa: E402
from exact_data import exact_equal                                          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
F32, I32 = torch.float32, torch.int32
DT = pytest.mark.parametrize('dt', R.STORAGE, ids=R.STORAGE_IDS)
L1 = pytest.mark.parametrize('l1', [False, True], ids=['l2', 'l1'])
T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


@pytest.fixture(scope='module', autouse=True)
def _release_cases():
    yield
    R.clear_cache()


@pytest.fixture(autouse=True)
def _guards_intact():
    """After every test: no kernel wrote outside a tensor it was handed (tests/guarded.py)."""
    guarded.reset()
    yield
    guarded.check_guards()


def dev(t):
    return guarded.inp(t, DEV, depth=2)


def put(v64, dt, ld=None):
    """Exact f64 data as a guarded operand of type dt (asserted representable); rows `ld` wide when given, the columns [c, ld) NaN."""
    t = R.store(v64, dt)
    assert torch.equal(t.double(), T64(v64)), 'not representable in %s' % dt
    if ld is not None and ld != t.shape[-1]:
        o = torch.full(tuple(t.shape[:-1]) + (ld,), NAN, dtype=t.dtype)
        o[..., :t.shape[-1]] = t
        t = o
    return guarded.inp(t, DEV, depth=2)


def gout(shape, dt, fill=None):
    return guarded.out(shape, dt, DEV, fill=fill, what=guarded._caller(1))


def vec(n, fill=None):
    return guarded.out((n,), F32, DEV, fill=fill, what=guarded._caller(1))


def same(got, v64, dt, what):
    """got holds, bit for bit, what a kernel stores for v64: the nearest f32 value, rounded once more (RNE) to a 16-bit dt."""
    want = R.stored_bits(v64, dt)
    exact_equal(got, want, what, exact=T64(v64) if want.dtype == torch.int16 else None)


def total(part, ref, what):
    """The partials, every one finite, sum (f64, on the host) to the exact value."""
    assert bool(torch.isfinite(part).all()), '%s: a partial is not finite' % what
    exact_equal(part.double().sum().reshape(1).cpu(), T64([ref]), what)


def held(got, ref, bound, what, keep=None):
    """No element outside its bound; returns the largest err/bound."""
    got = R.widen(got).reshape(np.shape(ref))
    bad = R.violations(got, ref, bound)
    ref, bound = np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    if keep is not None:
        bad &= keep
        got, ref, bound = got[keep], ref[keep], bound[keep]
    r = R.ratio(got, ref, bound)
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError('%s: %d/%d elements outside their bound (%d not finite), largest err/bound %.3g, first at %s' % (
            what, int(bad.sum()), bad.size, int((~np.isfinite(got)).sum()), r, i))
    return r


# ==============================================================================================
# A. error sums, exact
# ==============================================================================================
@DT
@L1
def test_masked_sse_exact(ops, dt, l1):
    from imm_amd import _lib as L
    e = R.sse_case()
    B, S = R.SSE_B, R.SSE_S
    md = put(e.mask, F32)
    for (s, c), (a, b) in zip(R.SSE_FEATS, e.feats):
        ad, bd = put(a, dt), put(b, dt)
        for mk, mkd in ((e.mask, md), (None, None)):
            part = vec(L.SSE_BLOCKS)
            ops.masked_sse(ad, bd, B, s, c, mkd, S, part, l1=l1)
            torch.cuda.synchronize()
            total(part, R.sse(a, b, mk, S, s, l1), 'masked_sse s%d c%d %s' % (s, c, 'masked' if mk is not None else 'no mask'))


@DT
@L1
@pytest.mark.parametrize('n', [1, 8])
def test_masked_sse_multi_and_all_exact(ops, n, dt, l1):
    """Rows f < n of a NaN-filled partial table are overwritten, the rows beyond stay untouched; the image slot of
    imm_masked_sse_all on a small pair (lda 3, ldb 16)."""
    from imm_amd import _lib as L
    e = R.sse_case()
    B, S = R.SSE_B, R.SSE_S
    md = put(e.mask, F32)
    ops_d = [(put(a, dt), put(b, dt)) for a, b in e.feats[:n]]
    img = R.image_case(B, S)
    ia, ib = put(img.a, F32), put(img.b, F32, 16)
    for mk, mkd in ((e.mask, md), (None, None)):
        tag = 'n%d %s' % (n, 'masked' if mk is not None else 'no mask')
        refs = [R.sse(a, b, mk, S, s, l1) for (s, c), (a, b) in zip(R.SSE_FEATS[:n], e.feats)]
        for fused in (False, True):
            table = gout((9, L.SSE_BLOCKS), F32)
            g = ops.SseMulti([(ad, bd, s, c, table[i]) for i, ((s, c), (ad, bd)) in enumerate(zip(R.SSE_FEATS[:n], ops_d))])
            if fused:
                ip = vec(L.SSE_BLOCKS)
                ops.masked_sse_all(g, B, mkd, S, ia, 3, ib, 16, 3, ip, l1=l1)
            else:
                ops.masked_sse_multi(g, B, mkd, S, l1=l1)
            torch.cuda.synchronize()
            name = 'masked_sse_all' if fused else 'masked_sse_multi'
            for i in range(n):
                total(table[i], refs[i], '%s %s feature %d' % (name, tag, i))
            assert untouched(table[n:]), '%s %s: a partial row of a feature that is not in the launch was written' % (name, tag)
            if fused:
                total(ip, R.sse(img.a, img.b, mk, S, S, l1), 'masked_sse_all %s image' % tag)


@L1
@pytest.mark.parametrize('lda,ldb,shifted', R.IMG_LD, ids=R.IMG_IDS)
def test_masked_sse_f32_four_pixel_pass_exact(ops, lda, ldb, shifted, l1):
    """B 7, S 256: a quarter of the threads take the unrolled pass once, all take the plain loop.  Wide columns hold NaN; `shifted`
    operands start one float into their buffer (no 16-byte alignment: the scalar loads of the float4 branches' fallback)."""
    from imm_amd import _lib as L
    B, S = R.IMG_B, R.IMG_S
    e = R.image_case()
    npix = B * S * S
    assert npix > 3 * L.SSE_BLOCKS * 256 and npix < 4 * L.SSE_BLOCKS * 256

    def operand(v, ld):
        t = put(v.reshape(npix, 3), F32, ld)
        if not shifted:
            return t
        buf = gout((npix * ld + 4,), F32)
        view = buf[1:1 + npix * ld]
        view.copy_(t.reshape(-1))
        assert view.data_ptr() % 16 == 4
        return view

    a, b, md = operand(e.a, lda), operand(e.b, ldb), put(e.mask, F32)
    feat = put(R.ints(np.random.RandomState(5), (B, 8, 8, 8), -3, 3), torch.bfloat16)
    for mk, mkd in ((e.mask, md), (None, None)):
        ref = R.sse(e.a, e.b, mk, S, S, l1)
        part = vec(L.SSE_BLOCKS)
        ops.masked_sse_f32(a, lda, b, ldb, B, S, 3, mkd, part, l1=l1)
        torch.cuda.synchronize()
        total(part, ref, 'masked_sse_f32 lda%d ldb%d %s' % (lda, ldb, 'masked' if mk is not None else 'no mask'))
        part, fp = vec(L.SSE_BLOCKS), vec(L.SSE_BLOCKS)
        ops.masked_sse_all(ops.SseMulti([(feat, feat, 8, 8, fp)]), B, mkd, S, a, lda, b, ldb, 3, part, l1=l1)
        torch.cuda.synchronize()
        total(part, ref, 'masked_sse_all image slot lda%d ldb%d' % (lda, ldb))
        total(fp, 0.0, 'masked_sse_all: a feature against itself')


@L1
@pytest.mark.parametrize('c,lda,ldb', R.SMALL_C)
def test_masked_sse_f32_general_channels_exact(ops, c, lda, ldb, l1):
    from imm_amd import _lib as L
    e = R.image_case(2, 8, c)
    a, b, md = put(e.a.reshape(-1, c), F32, lda), put(e.b.reshape(-1, c), F32, ldb), put(e.mask, F32)
    for mk, mkd in ((e.mask, md), (None, None)):
        part = vec(L.SSE_BLOCKS)
        ops.masked_sse_f32(a, lda, b, ldb, 2, 8, c, mkd, part, l1=l1)
        torch.cuda.synchronize()
        total(part, R.sse(e.a, e.b, mk, 8, 8, l1), 'masked_sse_f32 c%d' % c)


@DT
def test_masked_sse_pool_exact(ops, dt):
    """The case of tests/test_exact_gpu.py (r = 2), and r = 1, no mask and pool_a = None: the sum and the pooled halves."""
    from imm_amd import _lib as L
    B, s, c, S = E.SSE_SHAPE
    a, b, mask = (t.numpy() for t in E.sse_data(torch.bfloat16 if dt == F32 else dt))
    ad, bd = put(a, dt), put(b, dt)
    for mk, side in ((mask, S), (np.ascontiguousarray(mask[:, :s, :s]), s), (None, S)):
        ref = R.sse(a, b, mk, side, s, False)
        for with_a in (True, False):
            part = vec(L.SSE_BLOCKS)
            pa, pb = (gout((B, s // 2, s // 2, c), dt) if with_a else None), gout((B, s // 2, s // 2, c), dt)
            ops.masked_sse_pool(ad, bd, B, s, c, None if mk is None else put(mk, F32), side, part, pa, pb)
            torch.cuda.synchronize()
            total(part, ref, 'masked_sse_pool r%d' % (side // s))
            for got, src, what in ((pa, a, 'pool_a'), (pb, b, 'pool_b')):
                if got is not None:
                    same(got, src.reshape(B, s // 2, 2, s // 2, 2, c).max(axis=(2, 4)), dt, 'masked_sse_pool/' + what)


# ==============================================================================================
# B. perceptual_finalize
# ==============================================================================================
@pytest.mark.parametrize('nfeat', R.FINALIZE_NFEAT)
def test_perceptual_finalize_sums_in_f64_exact(ops, nfeat):
    """m[f] = (float)(sum / nel) bit for bit, on rows whose f32 sum is not the exact one and that differ from feature to feature."""
    part, nel = R.finalize_exact_table(nfeat)
    out, agg = vec(3 * nfeat + 3), vec(nfeat, fill=1.0)
    ops.perceptual_finalize(dev(torch.from_numpy(part)), nfeat, dev(torch.from_numpy(nel)), agg, True, None, out)
    torch.cuda.synchronize()
    m = (part.astype(np.float64).sum(1) / nel).astype(np.float32)
    exact_equal(out[nfeat:2 * nfeat], torch.from_numpy(m), 'perceptual_finalize m, nfeat %d' % nfeat)


@L1
@pytest.mark.parametrize('training', [1, 0], ids=['training', 'eval'])
@pytest.mark.parametrize('nfeat', R.FINALIZE_NFEAT)
def test_perceptual_finalize_bounded(ops, nfeat, training, l1):
    part, nel, agg0, wd = R.finalize_real_case(nfeat)
    pd, nd, wdd = dev(torch.from_numpy(part)), dev(torch.from_numpy(nel)), dev(torch.tensor([float(wd)]))
    outs, worst = [], 0.0
    for S in (None, 256.0):
        agg, out = vec(nfeat, fill=torch.from_numpy(agg0)), vec(3 * nfeat + 3)
        ops.perceptual_finalize(pd, nfeat, nd, agg, training, wdd, out, l1, ops.LOSS_PERCEPTUAL,
                                None if S is None else dev(torch.tensor([S, 0.0, 0.0, 0.0])))
        torch.cuda.synchronize()
        ref, ref_agg = R.finalize(part, nel, agg0, training, wd, l1, R.LOSS_PERCEPTUAL, S)
        b, b_agg = R.finalize_bounds(part, nel, agg0, training, wd, l1, R.LOSS_PERCEPTUAL, S)
        worst = max(worst, held(out, ref, b, 'finalize out (scale %s)' % S), held(agg, ref_agg, b_agg, 'finalize agg'))
        if not training:
            exact_equal(agg, torch.from_numpy(agg0), 'eval must leave agg as it was')
        outs.append(out.cpu())
    a, b = outs
    n = nfeat
    assert torch.equal(a[:2 * n], b[:2 * n]) and torch.equal(a[3 * n:], b[3 * n:]), 'the loss scale moved a loss value'
    assert torch.equal(a[2 * n:3 * n] * 256.0, b[2 * n:3 * n]), 'the loss scale must multiply the coefficients exactly'
    print('perceptual_finalize nfeat %d: largest err/bound %.3f' % (nfeat, worst))


def test_perceptual_finalize_l2_mode_bounded(ops):
    part, nel, agg0, wd = R.finalize_real_case(1, seed=3)
    pd, nd, wdd = dev(torch.from_numpy(part)), dev(torch.from_numpy(nel)), dev(torch.tensor([float(wd)]))
    outs, worst = [], 0.0
    for S in (None, 256.0):
        agg, out = vec(1, fill=torch.from_numpy(agg0)), vec(6)
        ops.perceptual_finalize(pd, 1, nd, agg, 1, wdd, out, False, ops.LOSS_L2, None if S is None else dev(torch.tensor([S, 0.0, 0.0, 0.0])))
        torch.cuda.synchronize()
        ref, _ = R.finalize(part, nel, agg0, 1, wd, False, R.LOSS_L2, S)
        b, _ = R.finalize_bounds(part, nel, agg0, 1, wd, False, R.LOSS_L2, S)
        worst = max(worst, held(out, ref, b, 'finalize L2 out (scale %s)' % S))
        exact_equal(agg, torch.from_numpy(agg0), 'the L2 mode has no normaliser: agg stays')
        outs.append(out.cpu())
    a, b = outs
    assert torch.equal(a[:2], b[:2]) and torch.equal(a[3:], b[3:]) and float(a[2]) * 256.0 == float(b[2])
    print('perceptual_finalize L2 mode: largest err/bound %.3f' % worst)


# ==============================================================================================
# C. gradient injection, exact
# ==============================================================================================
@DT
@L1
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
@pytest.mark.parametrize('has_in', [True, False], ids=['accumulate', 'fresh'])
def test_tap_grad_exact(ops, has_in, relu, l1, dt):
    e = R.tap_case(dt)
    B, s, c = R.TAP_B, R.TAP_S, R.TAP_C
    apd, agd = put(e.ap, dt), put(e.ag, dt)
    coef = dev(torch.tensor([NAN, NAN, R.TAP_COEF, NAN]))
    for S in R.TAP_MASK_SIDE:
        mk = e.masks[S] if S else None
        da = gout((B, s, s, c), dt, fill=R.store(e.d, dt) if has_in else None)
        ops.tap_grad(da, has_in, apd, agd, B, s, c, None if mk is None else put(mk, F32), S or s, coef, 2, relu, l1)
        torch.cuda.synchronize()
        same(da, R.tap_grad(e.d if has_in else None, e.ap, e.ag, mk, S or s, R.TAP_COEF, relu, l1), dt, 'tap_grad mask side %s' % S)


@DT
def test_unpool_tap_grad_exact(ops, dt):
    e = R.unpool_case(dt)
    B, s, c = R.UNPOOL_B, R.UNPOOL_S, R.UNPOOL_C
    apd, agd, dpd = put(e.ap, dt), put(e.ag, dt), put(e.dpool, dt)
    coef = dev(torch.tensor([NAN, R.UNPOOL_COEF[dt], NAN]))
    for S in (None, 16, 32):
        mk = e.masks[S] if S else None
        da = gout((B, s, s, c), dt)
        ops.unpool_tap_grad(da, dpd, apd, agd, B, s, c, None if mk is None else put(mk, F32), S or s, coef, 1)
        torch.cuda.synchronize()
        same(da, R.unpool_tap_grad(e.dpool, e.ap, e.ag, mk, S or s, R.UNPOOL_COEF[dt]), dt, 'unpool_tap_grad mask side %s' % S)


@DT
@L1
@pytest.mark.parametrize('ldp,lddp', [(3, 8), (16, 16), (3, 16), (16, 8)])
def test_image_loss_grad_exact(ops, ldp, lddp, l1, dt):
    e = R.imgrad_case()
    ck = R.IMG_COEF[dt]
    gt, pred = put(e.gt, F32), put(e.pred, F32, ldp)
    coef = dev(torch.tensor([NAN, ck]))
    for mk in (e.mask, None):
        dp = gout((e.gt.shape[0], lddp), dt)
        ops.image_loss_grad(gt, pred, ldp, R.IMGRAD_B, R.IMGRAD_S, None if mk is None else put(mk, F32), coef, 1, dp, lddp, l1)
        torch.cuda.synchronize()
        same(dp, R.image_loss_grad(e.gt, e.pred, mk, ck, l1, lddp), dt, 'image_loss_grad ldp%d lddp%d' % (ldp, lddp))
        assert bool((dp[:, 3:].contiguous().view(torch.int16 if dp.element_size() == 2 else I32) == 0).all()), 'channels >= 3 must be +0'


# ==============================================================================================
# D. optimizer
# ==============================================================================================
HP_FIELDS = ('lr_start', 'lr_decay', 'lr_step', 'lr_multiple', 'beta1', 'beta2', 'eps', 'clip', 'grad_scale', 'optim',
             'scale_growth_interval', 'scale_max')


def hp_of(ops, hp):
    return ops.OptHParams(**{k: getattr(hp, k) for k in HP_FIELDS})


def put32(v64):
    t = torch.from_numpy(np.ascontiguousarray(v64, dtype=np.float64)).float()
    assert torch.equal(t.double(), T64(v64)), 'not an f32 value'
    return guarded.inp(t, DEV, depth=2)


def opt_state(ops, e, w, m, v, gs=0, t=0):
    tab = ops.SegmentTable([int(n) for n in np.diff(e.tab.offsets)], [float(x) for x in e.wd], DEV)
    assert tab.nblk == e.tab.nblk and tab.nseg == e.tab.nseg
    return SimpleNamespace(tab=tab, params=put32(w), m=put32(m), v=put32(v), part=vec(tab.nblk), norm2=vec(tab.nseg), lrs=vec(2),
                           step=guarded.out((1,), I32, DEV, fill=gs), adam_t=guarded.out((1,), I32, DEV, fill=t))


def opt_run(ops, st, g, hp, ls=None):
    grads = put32(g)
    ops.clip_adam_step(st.params, grads, st.m, st.v, st.tab, st.part, st.norm2, st.step, st.adam_t, st.lrs, hp_of(ops, hp), ls)
    torch.cuda.synchronize()
    return grads


def exact32(got, v64, what):
    v = np.asarray(v64, np.float64)
    assert R.exact_in_f32(v), what + ': the reference is not an f32 value'
    exact_equal(got, torch.from_numpy((v + 0.0).astype(np.float32)), what)


def norm2_is_the_f64_sum(st, tab, what):
    want = R.norms(tab, R.widen(st.part)).astype(np.float32)
    exact_equal(st.norm2, torch.from_numpy(want), what + ': seg_norm2 is not (float) of the f64 sum of the tensor\'s chunk sums')


def test_optimizer_one_exact_step(ops):
    e = R.exact_opt_case()
    st = opt_state(ops, e, e.w, e.m, e.v)
    wdl, wpart = vec(1), vec(e.tab.nblk)
    ops.weight_decay_loss(st.params, st.tab, wpart, wdl)
    torch.cuda.synchronize()
    p, tot = R.weight_decay_loss(e.w, e.wd, e.tab)
    exact32(wpart, p, 'weight_decay_loss chunk sums')
    assert bool((wpart.cpu()[torch.from_numpy(e.wd[e.tab.seg] == 0)] == 0).all()), 'a wd == 0 tensor has a weight-decay term'
    exact_equal(wdl, torch.from_numpy(np.asarray([tot]).astype(np.float32)), 'weight_decay_loss')
    grads = opt_run(ops, st, e.g, e.hp)
    r = R.step(e.hp, e.tab, e.wd, e.g, e.w, e.m, e.v, 0, 0)
    exact32(grads, r.grads, 'prepared gradients')
    exact32(st.part, r.blk_partial, 'chunk sums of the squared gradients')
    exact_equal(st.norm2, torch.from_numpy(r.norm2.astype(np.float32)), 'seg_norm2')
    exact32(st.m, r.m, 'm')
    exact32(st.v, r.v, 'v')
    worst = held(st.params, r.w, r.e_w, 'params')
    assert int(st.step) == 1 and int(st.adam_t) == 1
    print('optimizer, one exact step: params largest err/bound %.3f' % worst)


def test_optimizer_default_prologue_beyond_256_chunks(ops):
    """No loss scale, production CHUNK: a workgroup scans its own tensor's chunk sums only, from the first index = tid (mod 256) at
    or after the tensor's first chunk.  The same table with a loss scale of 1 takes the full scan: bit-identical results."""
    e = R.prologue_case()
    assert R.CHUNK == ops.SegmentTable.CHUNK
    res = []
    for with_ls in (False, True):
        st = opt_state(ops, e, e.w, e.m, e.v)
        ls = dev(torch.tensor([1.0, 0.0, 0.0, 0.0])) if with_ls else None
        grads = opt_run(ops, st, e.g, e.hp, ls)
        res.append((st, grads))
    st, grads = res[0]
    r = R.step(e.hp, e.tab, e.wd, e.g, e.w, e.m, e.v, 0, 0)
    exact32(grads, r.grads, 'prepared gradients')
    exact32(st.part, r.blk_partial, 'chunk sums')
    norm2_is_the_f64_sum(st, e.tab, 'own-tensor scan')
    exact_equal(st.norm2, torch.from_numpy(r.norm2.astype(np.float32)), 'seg_norm2')
    worst = max(held(st.m, r.m, r.e_m, 'm'), held(st.v, r.v, r.e_v, 'v'), held(st.params, r.w, r.e_w, 'params', ~r.left_out))
    o = e.tab.offsets
    z = slice(int(o[R.PRO_ZERO]), int(o[R.PRO_ZERO + 1]))
    for got, was, what in ((st.params, e.w, 'params'), (st.m, e.m, 'm'), (st.v, e.v, 'v')):
        exact32(got[z], was[z], 'the tensor with an all-zero gradient: ' + what)
    c = slice(int(o[R.PRO_AT_CLIP]), int(o[R.PRO_AT_CLIP + 1]))
    exact32(st.m[c], (1.0 - e.hp.beta1) * e.g[c], 'norm == clip is not clipped: m')
    for a, b, what in zip((st.params, st.m, st.v, st.norm2), (res[1][0].params, res[1][0].m, res[1][0].v, res[1][0].norm2),
                          ('params', 'm', 'v', 'seg_norm2')):
        assert torch.equal(a.view(I32), b.view(I32)), 'own-tensor scan and full scan differ in ' + what
    print('optimizer, default prologue: largest err/bound %.3f, left out %.4f %%' % (worst, 100.0 * r.left_out.mean()))


@pytest.mark.parametrize('name', list(R.REAL_RUNS))
def test_optimizer_three_steps_against_f64(ops, name):
    e = R.real_opt_case(name)
    st = opt_state(ops, e, e.w0, e.m0, e.v0)
    worst, left = 0.0, np.zeros(e.tab.total, bool)
    for it, r in enumerate(e.steps):
        grads = opt_run(ops, st, e.g, e.hp)
        tag = '%s step %d ' % (name, it)
        keep = ~left                                                        # what an earlier step left out carries no bound
        worst = max(worst, held(grads, r.grads, r.e_grads, tag + 'grads', keep), held(st.part, r.blk_partial, r.e_blk, tag + 'chunk sums',
                    np.add.reduceat(left.astype(int), e.tab.begin) == 0), held(st.m, r.m, r.e_m, tag + 'm', keep), held(st.v, r.v, r.e_v, tag + 'v', keep))
        norm2_is_the_f64_sum(st, e.tab, tag)
        left |= r.left_out
        worst = max(worst, held(st.params, r.w, r.e_w, tag + 'params', ~left))
    assert left.mean() <= R.LEFT_OUT_CAP
    assert int(st.step) == 3 and int(st.adam_t) == 3
    print('optimizer %s, three steps: largest err/bound %.3f, left out %.4f %%' % (name, worst, 100.0 * left.mean()))


@pytest.mark.parametrize('t', [0, 9])
@pytest.mark.parametrize('k', [-1, 0, 1], ids=['lr_step-1', 'lr_step', '2lr_step'])
def test_learning_rate_against_f64(ops, k, t):
    lr_step = 1000
    gs = lr_step - 1 if k < 0 else (k + 1) * lr_step
    hp = R.hparams(lr_step=lr_step, lr_multiple=0.5)
    e = SimpleNamespace(tab=R.chunks([5]), wd=np.zeros(1))
    z = np.zeros(5)
    st = opt_state(ops, e, z, z, z, gs=gs, t=t)
    opt_run(ops, st, np.ones(5), hp)
    ref = np.asarray(R.learning_rate(hp, gs, t))
    got = R.widen(st.lrs)
    err = np.abs(got - ref) / R.ulp32(ref)
    print('lr_state at global_step %d, t %d: %.3f and %.3f ulp' % (gs, t, err[0], err[1]))
    assert (err <= 2.0).all(), (got, ref, err)
    assert int(st.step) == gs + 1 and int(st.adam_t) == t + 1


def test_skip_rule_on_a_finite_absurd_gradient(ops):
    """One finite gradient whose square exceeds IMM_NORM2_SANE: with a loss scale the whole step is skipped and S halves; without
    one the step proceeds and the tensor is clipped."""
    e = SimpleNamespace(tab=R.chunks([5, 3]), wd=np.zeros(2))
    hp = R.hparams(clip=1.0)
    g = np.asarray([1.0, -2.0, 2.0 ** 52, 3.0, 0.0, 1.0, 2.0, -1.0])
    w = np.arange(8) / 4.0
    assert np.isfinite(np.float32((g[2] / 2) ** 2)) and (g[2] / 2) ** 2 > R.NORM2_SANE
    st = opt_state(ops, e, w, np.zeros(8), np.zeros(8))
    ls = dev(torch.tensor([2.0, 0.0, 0.0, 0.0]))
    opt_run(ops, st, g, hp, ls)
    for got, was, what in ((st.params, w, 'params'), (st.m, np.zeros(8), 'm'), (st.v, np.zeros(8), 'v')):
        exact32(got, was, 'a skipped step must leave %s as it was' % what)
    assert int(st.step) == 0 and int(st.adam_t) == 0 and ls.tolist() == [1.0, 0.0, 1.0, 1.0]
    st = opt_state(ops, e, w, np.zeros(8), np.zeros(8))
    opt_run(ops, st, g / 2, hp)
    r = R.step(hp, e.tab, e.wd, g / 2, w, np.zeros(8), np.zeros(8), 0, 0)
    assert r.factor[0] < 1e-15 and r.factor[1] < 1.0
    norm2_is_the_f64_sum(st, e.tab, 'no loss scale')
    worst = max(held(st.m, r.m, r.e_m, 'm'), held(st.v, r.v, r.e_v, 'v'), held(st.params, r.w, r.e_w, 'params', ~r.left_out))
    assert int(st.step) == 1 and int(st.adam_t) == 1 and not r.left_out[2]
    print('skip rule, the step without a loss scale: largest err/bound %.3f' % worst)
