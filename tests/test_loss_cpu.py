"""tests/loss_reference.py and the data of tests/test_loss_gpu.py, pinned without a GPU.

  the reference   agrees with oracle/imm_oracle.py (exp_running_avg, loss_mask_at, clip_by_norm, adam_apply, adadelta_apply,
                  adagrad_apply, learning_rate, weight_decay_loss) and with torch autograd (the coefficients of finalize, the
                  gradient at a tap, max_pool2d's tie rule) on small cases.
  exact data      every exact case of the GPU module meets its premise: operands representable in the storage type, every
                  workgroup's sum of |terms| below 2^24, 16-bit outputs that round (>= 20 % not representable, >= 5 % ties, >= 5 %
                  inexact non-ties), the edges each case is there for (a different mask per sample, pixels on the ReLU edge and
                  with ap == ag, positive ties in the pooling windows, chunk heads and tails at all four offsets, ...).
  bounded data    at most 1 % of the elements of a bounded case are left out, and every bound is finite.
"""
import math
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import imm_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as E                                                       # noqa: E402
import loss_reference as R                                                   # noqa: E402

DT = pytest.mark.parametrize('dt', R.STORAGE, ids=R.STORAGE_IDS)
T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731


@pytest.fixture(scope='module', autouse=True)
def _release_cases():
    yield
    R.clear_cache()


def representable(v, dt):
    return bool(torch.equal(R.store(v, dt).double(), T64(v)))


def is_16bit_exercised(v, dt, what):
    """The mix tests/test_exact_cpu.py asks of a 16-bit output."""
    n_inexact, n_tie, n_other = E.rounding_mix(T64(v), dt)
    assert n_inexact >= 0.20 and n_tie >= 0.05 and n_other >= 0.05, \
        '%s: %.1f %% not representable, %.1f %% ties, %.1f %% inexact non-ties (need 20 / 5 / 5)' % (
            what, 100 * n_inexact, 100 * n_tie, 100 * n_other)


# ---- the reference against the oracle and autograd --------------------------------------------
def test_finalize_equals_the_oracle_and_autograd():
    part, nel, agg, wd = R.finalize_real_case(6)
    for l1 in (False, True):
        out, new = R.finalize(part, nel, agg, 1, wd, l1, R.LOSS_PERCEPTUAL, 256.0)
        n = 6
        m = torch.tensor(part.astype(np.float64).sum(1) / nel.astype(np.float64), requires_grad=True)
        wl = O.exp_running_avg(m, T64(agg))
        (1000.0 * (m / wl).sum()).backward()
        np.testing.assert_allclose(new, wl.detach().numpy(), rtol=1e-7)
        np.testing.assert_allclose(out[:n], (m / wl).detach().numpy(), rtol=1e-7)
        np.testing.assert_allclose(out[2 * n:3 * n], 256.0 * m.grad.numpy() * (1 if l1 else 2) / nel.astype(np.float64), rtol=1e-6)
        np.testing.assert_allclose(out[3 * n + 2], 1000.0 * float((m / wl).detach().sum()) + float(wd), rtol=1e-7)
    assert np.array_equal(R.finalize(part, nel, agg, 0, wd, False, R.LOSS_PERCEPTUAL)[1], agg.astype(np.float64))
    o2, _ = R.finalize(part[:1], nel[:1], agg[:1], 1, wd, False, R.LOSS_L2)
    n0, w0 = float(nel[0]), float(wd)
    m0 = float(part[0].astype(np.float64).sum()) / n0
    np.testing.assert_allclose(o2, [m0, m0, 1000.0 / 255.0 * 2.0 / n0, 1000.0 * m0, w0, 1000.0 * m0 / 255.0 + w0], rtol=1e-15)


def test_mask_pick_and_sse_equal_the_oracle():
    e = R.sse_case()
    for (s, c), (a, b) in zip(R.SSE_FEATS, e.feats):
        mk = O.loss_mask_at(T64(e.mask).unsqueeze(-1), s)
        assert np.array_equal(mk[..., 0].numpy(), R.pick(e.mask, R.SSE_S, s))
        assert R.sse(a, b, e.mask, R.SSE_S, s, False) == float(((T64(a) - T64(b)) ** 2 * mk).sum())
        assert R.sse(a, b, e.mask, R.SSE_S, s, True) == float(((T64(a) - T64(b)).abs() * mk).sum())
    assert len({R.SSE_S // s for s, _c in R.SSE_FEATS}) == 4 and {c // 8 for _s, c in R.SSE_FEATS} == {1, 17}


@pytest.mark.parametrize('l1', [False, True])
def test_tap_grad_equals_autograd(l1):
    e = R.tap_case(torch.float16)
    mask = e.masks[16]
    ap = T64(e.ap + 0.25).requires_grad_(True)                           # (off the |.| kink: autograd's sign(0) is a convention)
    mk = T64(R.pick(mask, 16, R.TAP_S)).unsqueeze(-1)
    d = ap - T64(e.ag)
    loss = R.TAP_COEF * ((d.abs() if l1 else 0.5 * d * d) * mk).sum()
    (g,) = torch.autograd.grad(loss, ap)
    want = (T64(e.d) + g) * (ap > 0)
    np.testing.assert_allclose(R.tap_grad(e.d, e.ap + 0.25, e.ag, mask, 16, R.TAP_COEF, True, l1), want.numpy(), rtol=0, atol=1e-12)


def test_pooling_tie_rule_is_torch_autograds():
    """The first maximum in the order (0,0), (0,1), (1,0), (1,1) takes the gradient: torch's max_pool2d on the CPU."""
    e = R.unpool_case(torch.float16)
    x = T64(e.ap).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = torch.nn.functional.max_pool2d(x, 2)
    (g,) = torch.autograd.grad(y, x, T64(e.dpool).permute(0, 3, 1, 2).contiguous())
    assert np.array_equal(g.permute(0, 2, 3, 1).numpy(), R.unpool(e.dpool, e.ap))
    _am, w = R.window_argmax(e.ap)
    assert bool(((w == w.max(3, keepdims=True)).sum(3) > 1).any())


def test_optimizer_equals_the_oracle():
    g0 = np.random.RandomState(3)
    sizes, wds = [40, 7, 3000], [O.WEIGHT_DECAY, 0.0, O.WEIGHT_DECAY]
    tab = R.chunks(sizes)
    names = ['a/w', 'b/b', 'c/w']
    w = g0.standard_normal(tab.total) * 0.3
    g = g0.standard_normal(tab.total) * R.per_seg(tab, [3.0, 1e-3, 0.5])
    split = lambda x: OrderedDict((k, T64(x[tab.offsets[i]:tab.offsets[i + 1]])) for i, k in enumerate(names))   # noqa: E731
    cat = lambda d: np.concatenate([v.numpy() for v in d.values()])                                             # noqa: E731
    p, tot = R.weight_decay_loss(w, wds, tab)
    np.testing.assert_allclose(tot, float(O.weight_decay_loss(split(w))), rtol=1e-12)
    for optim, kw in ((R.ADAM, {}), (R.ADADELTA, dict(beta1=0.95, eps=1e-6)), (R.ADAGRAD, {})):
        hp = R.hparams(optim=optim, grad_scale=0.5, clip=1.0, lr_start=1e-2, lr_step=2, **kw)
        P = split(w)
        opt = O.new_adam_state(P) if optim == R.ADAM else O.new_adagrad_state(P, R.r32(0.1))
        if optim == R.ADADELTA:
            opt = {'m': split(np.zeros(tab.total)), 'v': split(np.zeros(tab.total))}
        wr, m, v = w, np.zeros(tab.total), (np.full(tab.total, R.r32(0.1)) if optim == R.ADAGRAD else np.zeros(tab.total))
        for it in range(3):
            r = R.step(hp, tab, wds, 2.0 * g, wr, m, v, it, it, S=None)
            gref = {k: O.clip_by_norm(x + (O.WEIGHT_DECAY * P[k] if k.endswith('/w') else 0), 1.0) for k, x in split(g).items()}
            lr = O.learning_rate(it, hp.lr_start, 2, hp.lr_decay, hp.lr_multiple)
            np.testing.assert_allclose(r.lr, lr, rtol=1e-15)
            if optim == R.ADAM:
                P = O.adam_apply(P, gref, opt, lr, hp.beta1, hp.beta2, hp.eps)
            elif optim == R.ADADELTA:
                P = O.adadelta_apply(P, gref, opt, lr, hp.beta1, hp.eps)
            else:
                P = O.adagrad_apply(P, gref, opt, lr)
            np.testing.assert_allclose(r.gc, cat(gref), rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(r.w, cat(P), rtol=1e-12)
            np.testing.assert_allclose(r.v, cat(opt['v']), rtol=1e-12)
            wr, m, v = r.w, r.m, r.v
    # a loss scale divides the gradients again, exactly
    a = R.prepare(8.0 * g, w, wds, 0.5, 8.0, tab)[0]
    assert np.array_equal(a, R.prepare(g, w, wds, 0.5, None, tab)[0])


def test_chunk_table_is_the_segment_tables():
    from imm_amd import ops
    assert R.CHUNK == ops.SegmentTable.CHUNK
    for sizes in (R.EXACT_SIZES, R.PRO_SIZES, R.REAL_SIZES):
        t, d = R.chunks(sizes), ops.SegmentTable(sizes, [0.0] * len(sizes), 'cpu')
        assert (t.nblk, t.nseg, t.total) == (d.nblk, d.nseg, d.total) and list(t.offsets) == d.offsets
        for a, b in ((t.seg, d.blk_seg), (t.begin, d.blk_begin), (t.end, d.blk_end), (t.first, d.seg_first_blk)):
            assert a.tolist() == b.tolist()


# ---- exact data: the error sums ----------------------------------------------------------------
@DT
def test_sse_cases_are_exact(dt):
    e = R.sse_case()
    assert not np.array_equal(e.mask[0], e.mask[1]) and not np.array_equal(e.mask[1], e.mask[2]) and not np.array_equal(e.mask[0], e.mask[2])
    for (s, c), (a, b) in zip(R.SSE_FEATS, e.feats):
        assert representable(a, dt) and representable(b, dt)
        for l1 in (False, True):
            d = a - b
            t = (np.abs(d) if l1 else d * d).reshape(R.SSE_B, s, s, c // 8, 8).sum(-1) * R.pick(e.mask, R.SSE_S, s)[..., None]
            assert R.block_abs_sums(t).max() < R.LIMIT
            # a launch that read sample 0's mask for every sample, or the mask at stride 1, gives another sum
            wrong = np.broadcast_to(e.mask[:1], e.mask.shape)
            assert R.sse(a, b, wrong, R.SSE_S, s, l1) != R.sse(a, b, e.mask, R.SSE_S, s, l1)
            if s < R.SSE_S:
                assert float((t.sum(-1) / np.maximum(R.pick(e.mask, R.SSE_S, s), 1) * e.mask[:, :s, :s]).sum()) != R.sse(a, b, e.mask, R.SSE_S, s, l1)


def test_image_cases_are_exact():
    e = R.image_case()
    npix = R.IMG_B * R.IMG_S * R.IMG_S
    stride = R.SSE_BLOCKS * R.THREADS
    assert 3 * stride < npix < 4 * stride, 'the unrolled pass must run once for some threads and not at all for the others'
    for l1 in (False, True):
        t = R.sse_terms(e.a, e.b, e.mask, R.IMG_S, R.IMG_S, l1)
        assert R.block_abs_sums(t).max() < R.LIMIT
        # the mask of the first of the four pixels used for all four (the unrolled pass covers p < npix - 3 stride)
        p = np.arange(npix)
        first = np.where(p % stride < npix - 3 * stride, p % stride, p)
        raw = R.sse_terms(e.a, e.b, None, R.IMG_S, R.IMG_S, l1).reshape(-1)
        assert float((raw * e.mask.reshape(-1)[first]).sum()) != float(t.sum())
    for c, _lda, _ldb in R.SMALL_C:
        s = R.image_case(2, 8, c)
        assert R.block_abs_sums(R.sse_terms(s.a, s.b, s.mask, 8, 8, False)).max() < R.LIMIT


@DT
def test_pool_case_is_exact(dt):
    B, s, c, S = E.SSE_SHAPE
    a, b, mask = (t.numpy() for t in E.sse_data(torch.bfloat16 if dt == torch.float32 else dt))
    assert representable(a, dt) and representable(b, dt)
    d = a - b
    t = (d * d).reshape(B, s, s, c // 8, 8).sum(-1) * R.pick(mask, S, s)[..., None]
    t = t.reshape(B, s // 2, 2, s // 2, 2, c // 8).sum((2, 4))               # one item of the pooled launch: a window of four pixels
    assert R.block_abs_sums(t).max() < R.LIMIT


# ---- exact data: finalize ----------------------------------------------------------------------
@pytest.mark.parametrize('nfeat', R.FINALIZE_NFEAT)
def test_finalize_table_needs_f64(nfeat):
    part, nel = R.finalize_exact_table(nfeat)
    assert all(math.log2(float(n)).is_integer() for n in nel)
    want = []
    for f in range(nfeat):
        row = part[f].astype(np.float64)
        exact = math.fsum(row)
        assert exact == float(row.sum()) == float(row[::-1].sum()), 'the f64 sum must be exact in any order'
        m = np.float32(exact / float(nel[f]))
        want.append(float(m))
        for s32 in R.f32_sums(part[f]):
            assert np.float32(s32 / float(nel[f])) != m, 'an f32 sum reaches the same m: the row does not need f64'
    w = np.asarray(want)
    assert len(set(want)) == nfeat and (nfeat == 1 or w.max() / w.min() > 1e3 or nfeat < 16), 'rows must differ from feature to feature'


def test_finalize_bounds_are_finite_and_small():
    for nfeat in R.FINALIZE_NFEAT:
        part, nel, agg, wd = R.finalize_real_case(nfeat)
        for l1 in (False, True):
            out, _ = R.finalize(part, nel, agg, 1, wd, l1, R.LOSS_PERCEPTUAL, 256.0)
            b, ba = R.finalize_bounds(part, nel, agg, 1, wd, l1, R.LOSS_PERCEPTUAL, 256.0)
            assert np.isfinite(b).all() and (b <= 64 * R.U * np.abs(out)).all() and (ba > 0).all()
        mags = part.astype(np.float64).sum(1)
        assert nfeat == 1 or mags.max() / mags.min() > 10


# ---- exact data: gradient injection ------------------------------------------------------------
@DT
def test_tap_cases_are_exact(dt):
    e = R.tap_case(dt)
    assert all(representable(v, dt) for v in (e.ap, e.ag, e.d))
    assert (e.ap == e.ag).mean() > 0.05 and (e.ap == 0).mean() > 0.05 and (e.ap < 0).mean() > 0.2
    assert R.TAP_B * R.TAP_S * R.TAP_S * R.TAP_C // 8 > 256, 'more than one workgroup'
    for S, mk in e.masks.items():
        assert not np.array_equal(R.pick(mk, S, R.TAP_S)[0], R.pick(mk, S, R.TAP_S)[1])
        if S > R.TAP_S:
            assert not np.array_equal(R.pick(mk, S, R.TAP_S), mk[:, :R.TAP_S, :R.TAP_S]), 'the strided pick must differ from stride 1'
    for relu in (True, False):
        for l1 in (True, False):
            for S in R.TAP_MASK_SIDE:
                v = R.tap_grad(e.d, e.ap, e.ag, e.masks.get(S), S or R.TAP_S, R.TAP_COEF, relu, l1)
                assert R.exact_in_f32(v) and not np.signbit(v[v == 0]).any()
                if dt != torch.float32:                              # (behind the ReLU: the pixels it lets through)
                    is_16bit_exercised(v[e.ap > 0] if relu else v, dt, 'tap_grad relu=%s l1=%s S=%s' % (relu, l1, S))
                # without an incoming gradient v = coef mask e takes a few small values that every type holds: those runs pin the
                # term, the sign rule and the zero, the accumulating ones the rounding
                assert representable(R.tap_grad(None, e.ap, e.ag, e.masks.get(S), S or R.TAP_S, R.TAP_COEF, relu, l1), dt)
    # `>= 0` in place of `> 0` at the ReLU, or a sign(0) of +-1, each give another answer
    on_edge = (e.ap == 0) & (R.tap_grad(e.d, e.ap, e.ag, None, R.TAP_S, R.TAP_COEF, False, False) != 0)
    assert on_edge.mean() > 0.05


@DT
def test_unpool_cases_are_exact(dt):
    e = R.unpool_case(dt)
    assert all(representable(v, dt) for v in (e.ap, e.ag, e.dpool))
    am, w = R.window_argmax(e.ap)
    top = w.max(3)
    tie = ((w == top[:, :, :, None, :]).sum(3) > 1) & (top > 0)
    assert tie.mean() >= 0.05, 'positive ties for the maximum: %.1f %%' % (100 * tie.mean())
    assert (top <= 0).mean() > 0.01, 'windows that are all non-positive'
    assert (tie & (e.dpool != 0)).mean() >= 0.05, 'a tie shows only under a non-zero incoming gradient'
    for S in (None, 16, 32):
        v = R.unpool_tap_grad(e.dpool, e.ap, e.ag, e.masks.get(S), S or R.UNPOOL_S, R.UNPOOL_COEF[dt])
        assert R.exact_in_f32(v)
        if dt != torch.float32:
            is_16bit_exercised(v[e.ap > 0], dt, 'unpool_tap_grad S=%s (the pixels the ReLU lets through)' % S)


@DT
def test_image_grad_case_is_exact(dt):
    e = R.imgrad_case()
    assert (e.gt == e.pred).any() and R.IMGRAD_B * R.IMGRAD_S ** 2 > 256
    for mk in (e.mask, None):
        v = R.image_loss_grad(e.gt, e.pred, mk, R.IMG_COEF[dt], False, 8)
        assert R.exact_in_f32(v)
        if dt != torch.float32:
            is_16bit_exercised(v[:, :3], dt, 'image_loss_grad')


# ---- exact data: the optimizer -----------------------------------------------------------------
def test_exact_step_is_exact():
    e = R.exact_opt_case()
    assert sorted(R.EXACT_SIZES) == [1, 2, 3, 5, 2047, 2048, 2049, 4099]
    t = e.tab
    assert {int(b) % 4 for b in t.begin} == {0, 1, 2, 3} and {int(b) % 4 for b in t.end} == {0, 1, 2, 3}
    assert any(((int(b0) + 3) & ~3) > int(b1) for b0, b1 in zip(t.begin, t.end)), 'a chunk shorter than its head'
    r = R.step(e.hp, t, e.wd, e.g, e.w, e.m, e.v, 0, 0)
    for v in (e.g, e.w, e.m, e.v, r.grads, r.grads ** 2, r.blk_partial, r.gc, r.gc ** 2, r.m, r.v, 0.75 * e.v, 0.25 * r.gc ** 2):
        assert R.exact_in_f32(v)
    for b0, b1 in zip(t.begin, t.end):                                   # a chunk's squares are multiples of one power of two, and
        k = (r.grads[b0:b1] ** 2 * 2.0 ** 8).astype(np.int64)            # their sum stays below 2^24 of them: exact in any order
        unit = min((int(x) & -int(x)) for x in k if x) if k.any() else 1
        assert (r.grads[b0:b1] ** 2 * 2.0 ** 8 == k).all() and k.sum() // unit < R.LIMIT
    assert all(f == 1.0 or math.log2(f).is_integer() for f in r.factor) and (r.factor < 1).sum() == 3 and (r.factor == 1).sum() == 5
    assert all(math.sqrt(float(np.float32(n))) ** 2 == n or f == 1.0 for n, f in zip(r.norm2, r.factor)), 'sqrtf of a clipped norm is exact'
    has_wd = R.per_seg(t, e.wd) > 0
    ratio = np.abs(R.per_seg(t, e.wd) * e.w)[has_wd].mean() / np.abs(e.g * e.hp.grad_scale)[has_wd].mean()
    assert 0.25 < ratio < 4, ratio
    bare = R.step(e.hp, t, 0 * e.wd, e.g, e.w, e.m, e.v, 0, 0)
    for a, b in ((r.grads, bare.grads), (r.m, bare.m), (r.v, bare.v)):
        assert (a != b)[has_wd].mean() > 0.8, 'the decay term must be visible'
    p, _tot = R.weight_decay_loss(e.w, e.wd, t)
    assert R.exact_in_f32(p) and (p[e.wd[t.seg] == 0] == 0).all() and (p[e.wd[t.seg] > 0] > 0).all()


def test_prologue_case_reaches_the_own_tensor_scan():
    e = R.prologue_case()
    t = e.tab
    per = np.diff(t.first)
    big = np.flatnonzero(per > 256)
    assert len(big) == 2 and t.first[big[1]] >= 256 and big[0] > 0 and big[1] > big[0] + 1 and big[1] < t.nseg - 1
    r = R.step(e.hp, t, e.wd, e.g, e.w, e.m, e.v, 0, 0)
    assert all(R.exact_in_f32(v) for v in (e.g, e.w, r.grads, r.grads ** 2, r.blk_partial))
    for s in range(t.nseg):
        rows = r.blk_partial[t.first[s]:t.first[s + 1]]
        assert math.fsum(rows) == float(rows.sum()) == float(rows[::-1].sum()), 'the f64 sum of the chunk sums is exact in any order'
    nz = r.norm2[r.norm2 > 0]
    assert nz.max() / nz.min() > 1e12 and r.norm2[R.PRO_ZERO] == 0 and math.sqrt(r.norm2[R.PRO_AT_CLIP]) == e.hp.clip
    assert (r.factor < 1).sum() >= 2 and (r.factor == 1).sum() >= 3 and r.factor[R.PRO_AT_CLIP] == 1.0
    assert r.factor[big[0]] == 1.0 and r.factor[big[1]] < 1.0
    # a scan that starts one trip late loses chunks of both large tensors
    assert per[big[0]] > 256 and per[big[1]] > 256
    assert r.left_out.mean() <= R.LEFT_OUT_CAP
    assert all(np.isfinite(b).all() for b in (r.e_m, r.e_v, r.e_w))


@pytest.mark.parametrize('name', list(R.REAL_RUNS))
def test_real_runs_leave_out_at_most_one_percent(name):
    e = R.real_opt_case(name)
    left = np.zeros(e.tab.total, bool)
    for r in e.steps:
        left |= r.left_out
        assert all(np.isfinite(b).all() and (b >= 0).all() for b in (r.e_grads, r.e_blk, r.e_m, r.e_v, r.e_w))
        assert np.median(r.e_w[~left] / np.maximum(np.abs(r.w[~left]), 1e-30)) < 1e-5, 'a bound that bounds nothing'
    assert left.mean() <= R.LEFT_OUT_CAP, left.mean()
    f = e.steps[0].factor
    if e.hp.clip > 0:
        assert (f < 1).any() and (f == 1).any()
    else:
        assert (f == 1).all()
