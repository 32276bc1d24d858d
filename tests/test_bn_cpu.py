"""tests/bn_reference.py and the data of tests/test_bn_gpu.py, pinned without a GPU.

  the reference   equals torch.autograd in f64 through oracle.imm_oracle.batch_norm + ReLU (y, dgamma, dbeta, dy) to 1e-12.
  mutants         each deliberate change of the rule is rejected by bn_reference.violations() under the bounds the GPU test uses, on
                  the GPU test's own bounded inputs: in f32 storage on more than 25 % of the elements of at least one case.
                  16-bit storage adds half an ulp of the stored value (2^-9 bf16, 2^-12 f16 relative) to every bound, so the four
                  changes of relative size 1/N or eps/var are seen on fewer elements (worst case, f32 | bf16 | f16 storage):
                      N-1 for N in the mean            51 % | 27 % | 43 %
                      N-1 for N in k1 and k2           96 % | 66 % | 87 %
                      unbiased variance in rstd        50 % | 38 % | 43 %
                      eps dropped                      51 % |  4 % |  7 %     <- 16-bit storage cannot see this one
                  and at N = 4096 all four fall below 10 % in both 16-bit types.  That is why every bounded test also runs in f32
                  storage.  The dropped k1 term and the mask from y > 0 are O(1) changes, and the moving variance is an f32
                  output in every storage type: all types reject those on > 90 %.  `>= 0` for `> 0` shows only where
                  y sc + sh == 0 exactly, which real data never hits: it is rejected on the exact data, bit for bit.
  exact data      every case of section 1 of the GPU module meets its premise: operands representable in the storage type, every
                  product and every sum exact in f32 (below 2^24 units of its least bit), f32 sums in shuffled order equal to the
                  f64 sums, 16-bit results that round (ties and non-ties), >= 1 % of the pixels exactly on the ReLU edge.
  bounded data    an f32 numpy emulation of the documented arithmetic (sequential f32 sums per lane, then over the lanes; two
                  roundings per multiply-add) stays under every bound, and at most 0.1 % of the pixels of a case are left out.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import imm_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_reference as R                                                     # noqa: E402
from exact_data import rounding_mix                                          # noqa: E402

DT = pytest.mark.parametrize('dt', R.STORAGE, ids=R.STORAGE_IDS)
F32 = np.float32
T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731


@pytest.fixture(scope='module', autouse=True)
def _release_cases():
    """The cached cases (up to 32 776 x 256 f64 values each) are dropped when the module is done."""
    yield
    R.clear_cache()


# ---- the reference against autograd ----------------------------------------------------------
@pytest.mark.parametrize('c,npix', [(32, 1000), (64, 65)])
def test_reference_equals_autograd(c, npix, monkeypatch):
    e = R.bounded_case(c, npix, 1, torch.float32)
    y = T64(e.y).reshape(1, 1, npix, c).requires_grad_(True)
    g, b = T64(e.gamma).requires_grad_(True), T64(e.beta).requires_grad_(True)
    rows = np.stack([e.y.sum(0), (e.y ** 2).sum(0)])[None]
    st = R.stats(rows.astype(F32), npix)
    # the f64 sums themselves (the f32 rows carry their own rounding, which autograd does not see)
    st.mean, st.var = e.y.mean(0), e.y.var(0)
    st.rstd, st.unbiased = 1 / np.sqrt(st.var + float(R.EPS)), st.var * npix / (npix - 1)
    monkeypatch.setattr(O, 'BN_EPS', float(R.EPS))                       # the f32 values the kernels get, widened
    monkeypatch.setattr(O, 'BN_MOMENTUM', float(R.MOMENTUM))
    out, (mm, mv) = O.batch_norm(y, g, b, T64(e.mm), T64(e.mv), True)
    out = torch.relu(out)
    gy, gg, gb = torch.autograd.grad(out, [y, g, b], T64(e.dout).reshape(1, 1, npix, c))
    f = R.forward(e.y, e.gamma, e.beta, st)
    bw = R.backward(e.dout, e.y, f.scale, f.shift, st.mean, st.rstd, e.gamma, npix)
    rmm, rmv = R.moving(e.mm, e.mv, st, O.BN_MOMENTUM)
    for got, ref, what in ((f.out, out, 'y'), (bw.s2, gg, 'dgamma'), (bw.s1, gb, 'dbeta'), (bw.dy, gy, 'dy'), (rmm, mm, 'mm'), (rmv, mv, 'mv')):
        ref = ref.detach().numpy().reshape(got.shape)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), what


def test_half_ulp_covers_the_16_bit_store():
    """|RNE16(x) - x| <= half_ulp(|x|) with equality at ties, for normal and subnormal magnitudes."""
    x = np.concatenate([np.random.RandomState(0).standard_normal(4000) * 10.0 ** np.random.RandomState(1).randint(-9, 4, 4000),
                        [259.0, 257.0, 2049.0, 1e-7, 0.0]])
    for dt in R.STORAGE[:2]:
        err = np.abs(R.widen(R.store(x, dt)) - x.astype(F32).astype(np.float64))
        assert (err <= R.half_ulp(np.abs(x), dt)).all()
    assert R.half_ulp(np.array([257.0]), torch.bfloat16)[0] == 1.0 and R.half_ulp(np.array([2049.0]), torch.float16)[0] == 1.0
    assert R.half_ulp(np.array([3.0]), torch.float32)[0] == 0.0


# ---- mutants ----------------------------------------------------------------------------------
def _mutant_fwd(e, kind):
    n = e.npix
    S = e.rows.astype(np.float64).sum(0)
    with np.errstate(divide='ignore', invalid='ignore'):
        mean = S[0] / ((n - 1) if kind == 'mean_n1' else n)
        var = np.maximum(S[1] / n - mean * mean, 0.0)
        v = var * n / (n - 1) if kind == 'rstd_unbiased' else var
        rstd = 1 / np.sqrt(v + (0.0 if kind == 'no_eps' else float(R.EPS)))
        sc = e.gamma * rstd
        return np.maximum(e.y * sc + (e.beta - mean * sc), 0.0)


def _mutant_bwd(e, kind):
    n = e.npix
    r = R.backward(e.dout, e.y, e.scale, e.shift, e.mean, e.rstd, e.gamma, n)
    if kind == 'k_n1':
        return r.coef[0] * (r.dz - r.s1 / (n - 1) - r.xhat * r.s2 / (n - 1))
    if kind == 'no_k1':
        return r.coef[0] * (r.dz - r.xhat * r.coef[2])
    assert kind == 'mask_y'
    dz = e.dout * (e.y > 0)
    return r.coef[0] * (dz - dz.sum(0) / n - r.xhat * (dz * r.xhat).sum(0) / n)


MUTANTS = ['mean_n1', 'k_n1', 'rstd_unbiased', 'no_eps', 'no_k1', 'mask_y', 'moving_biased']
SMALL = ('mean_n1', 'k_n1', 'rstd_unbiased', 'no_eps')                       # changes of relative size 1/N or eps/var


def _worst_share(kind, dt):
    worst = 0.0
    for c, npix, nrows in R.BOUNDED_SHAPES:
        if npix == 1:
            continue                                         # N - 1 = 0
        e = R.bounded_case(c, npix, nrows, dt)
        if kind == 'moving_biased':
            b = R.forward_bounds(e.y, e.gamma, e.beta, e.st, e.mm, e.mv)
            ref = R.moving(e.mm, e.mv, e.st)[1]
            got = e.mv * float(R.MOMENTUM) + e.st.var * (1.0 - float(R.MOMENTUM))
            bad = R.violations(got, ref, b.moving_var)                       # an f32 output in every storage type
        elif kind in ('mean_n1', 'rstd_unbiased', 'no_eps'):
            b = R.forward_bounds(e.y, e.gamma, e.beta, e.st)
            bad = R.violations(_mutant_fwd(e, kind), e.fwd.out, b.out, dt)
        else:
            b = R.backward_bounds(e.dout, e.y, e.scale, e.shift, e.mean, e.rstd, e.gamma, npix, e.geo.L)
            bad = R.violations(_mutant_bwd(e, kind), b.ref.dy, b.dy, dt) & ~b.amb
        worst = max(worst, float(bad.mean()))
    return worst


@pytest.mark.parametrize('kind', MUTANTS)
def test_mutant_is_rejected_in_f32_storage(kind):
    share = _worst_share(kind, torch.float32)
    print('MUTANT %s f32: %.1f %% of the elements of its worst case break the bound' % (kind, 100 * share))
    assert share > 0.25, (kind, share)


@pytest.mark.parametrize('kind', MUTANTS)
def test_what_16_bit_storage_sees_of_a_mutant(kind):
    """The O(1) mutants and the f32 moving variance are rejected in every storage type; of the small ones 16-bit storage sees at
    most half of what f32 storage sees (the shares are printed: they are the table of the module's docstring)."""
    full = _worst_share(kind, torch.float32)
    for dt in R.STORAGE[:2]:
        share = _worst_share(kind, dt)
        print('MUTANT %s %s: %.1f %%' % (kind, str(dt)[6:], 100 * share))
        if kind in SMALL:
            assert share < full, (kind, dt, share, full)
        else:
            assert share > 0.25, (kind, dt, share)


@DT
def test_relu_edge_mutant_is_rejected_on_the_exact_data(dt):
    """`>= 0` for `> 0`: pixels exactly on the edge with dout != 0 change dz, so the exact sums and the exact dy differ."""
    hit = 0
    for c, npix in R.REDUCE_SHAPES:
        e = R.exact_case(c, npix)
        v = e.y * e.scale + e.shift
        r = R.backward(e.dout, e.y, e.scale, e.shift, e.mean, e.rstd, e.gamma, npix)
        dz = e.dout * (v >= 0)
        differs = bool((dz.sum(0) != r.s1).any() or ((dz * r.xhat).sum(0) != r.s2).any())
        dy_m = e.coef[0] * (dz - e.coef[1] - r.xhat * e.coef[2])
        dy = R.apply_coef(e.dout, e.y, e.scale, e.shift, e.mean, e.rstd, e.coef)
        differs_dy = not torch.equal(R.stored_bits(dy_m, dt), R.stored_bits(dy, dt))
        assert differs == differs_dy
        hit += differs
    assert hit >= len(R.REDUCE_SHAPES) - 1                  # (c 8, 1 pixel) may have no edge pixel with a gradient


# ---- exact data ------------------------------------------------------------------------------
def _shuffled_f32_sum(terms, seed):
    """Sequential f32 sum over the pixels in a random order (np.cumsum adds one element at a time in the array's own type)."""
    p = np.random.RandomState(seed).permutation(terms.shape[0])
    return np.cumsum(terms[p].astype(F32), axis=0, dtype=F32)[-1].astype(np.float64)


def _rounds(v64, dt, what):
    if dt == torch.float32 or v64.size < 1000:
        return
    inexact, tie, nontie = rounding_mix(T64(v64), dt)
    assert tie > 0.002 and nontie > 0.002, '%s: the %s store does not round both ways (%.4f not representable, %.4f ties, %.4f other)' % (
        what, dt, inexact, tie, nontie)


@DT
@pytest.mark.parametrize('c,npix', R.APPLY_SHAPES)
def test_exact_forward_data(c, npix, dt):
    e = R.exact_case(c, npix, R.Y_AMP[dt])
    assert torch.equal(R.store(e.y, dt).double(), T64(e.y)), 'y must be representable in %s' % dt
    for a in (e.scale, e.shift, e.mean, e.rstd, e.gamma, e.beta, e.y * e.scale, e.y * e.scale + e.shift):
        assert R.exact_in_f32(a)
    assert e.gamma[1] < 0 and e.gamma[2] == 0
    v = e.y * e.scale + e.shift
    assert bool((np.log2(e.rstd) % 1 == 0).all()) and bool((e.mean % 1 == 0).all())
    if npix >= 64:
        assert (v == 0).mean() >= 0.01, 'at least 1 %% of the pixels on the ReLU edge, got %.4f' % (v == 0).mean()
        _rounds(v, dt, 'apply c%d' % c)
        _rounds(np.maximum(v, 0), dt, 'apply+relu c%d' % c)
    assert np.abs(v).max() <= torch.finfo(dt).max / 2


@DT
@pytest.mark.parametrize('c,npix', sorted(set(R.APPLY_SHAPES + R.REDUCE_SHAPES)))
def test_exact_backward_data(c, npix, dt):
    e = R.exact_case(c, npix)
    assert torch.equal(R.store(e.y, dt).double(), T64(e.y)) and torch.equal(R.store(e.dout, dt).double(), T64(e.dout))
    for relu in (True, False):
        r = R.backward(e.dout, e.y, e.scale, e.shift, e.mean, e.rstd, e.gamma, npix, relu)
        terms = r.dz * r.xhat
        assert R.exact_in_f32(r.xhat) and R.exact_in_f32(terms)
        unit = 0.25 * 0.25                                              # xhat is a multiple of rstd >= 1/4; so is every partial sum
        assert np.abs(r.dz).sum(0).max() < 2 ** 24 and np.abs(terms).sum(0).max() / unit < 2 ** 24
        assert (_shuffled_f32_sum(r.dz, 1) == r.s1).all() and (_shuffled_f32_sum(terms, 2) == r.s2).all()
        # imm_bn_bwd_apply with the hand-made coef: every intermediate and the result exact in f32
        t = r.dz - e.coef[1] - r.xhat * e.coef[2]
        assert R.exact_in_f32(r.xhat * e.coef[2]) and R.exact_in_f32(r.dz - e.coef[1]) and R.exact_in_f32(t) and R.exact_in_f32(e.coef[0] * t)
        if npix >= 64:
            _rounds(e.coef[0] * t, dt, 'bwd_apply c%d' % c)
    if npix >= 64:
        assert ((e.y * e.scale + e.shift == 0) & (e.dout != 0)).mean() >= 0.01


@pytest.mark.parametrize('c,count,nblk', R.FUSED_CASES)
def test_exact_fused_backward_data(c, count, nblk):
    e = R.exact_case(c, count)
    S = R.fused_table(nblk, c).astype(np.float64).sum(0)
    k1, k2 = S[0] / count, S[1] / count
    assert R.exact_in_f32(k1) and R.exact_in_f32(k2) and R.exact_in_f32(S)
    r = R.backward(e.dout, e.y, e.scale, e.shift, e.mean, e.rstd, e.gamma, count)
    t = r.dz - k1 - r.xhat * k2
    assert R.exact_in_f32(r.dz - k1) and R.exact_in_f32(r.xhat * k2) and R.exact_in_f32(t), 'every step before the last product is exact'
    for dt in R.STORAGE[:2]:
        _rounds(np.float64(F32(e.scale * t)), dt, 'fused c%d' % c)


@pytest.mark.parametrize('c,nblk', R.FINALIZE_CASES)
def test_exact_tables(c, nblk):
    t = R.table(nblk, c, R.finalize_ldp(c))[:, :, :c]
    assert np.abs(t.astype(np.float64)).sum(0).max() < 2 ** 24 and bool((t % 1 == 0).all())
    assert (_shuffled_f32_sum(t.reshape(nblk, -1), 3) == t.astype(np.float64).sum(0).reshape(-1)).all()
    assert R.stats(t, nblk * 7).var.min() > 0                                  # not clamped
    # neighbouring rows differ in every channel pair somewhere: a row taken twice changes the totals
    if nblk > 1:
        assert bool((t[1:] != t[:-1]).any(axis=(1, 2)).all())


@pytest.mark.parametrize('B,h,w,c', R.UP_SHAPES)
def test_exact_upsampling_data(B, h, w, c):
    e = R.exact_up(B, h, w, c)
    up, adj = R.up_fwd(e.x), R.up_bwd(e.dy_up)
    assert bool((up % 1 == 0).all()) and bool((adj % 1 == 0).all()) and np.abs(adj).max() <= 256 and np.abs(up).max() <= 256
    # the adjoint identity <up_fwd(x), dy> == <x, up_bwd(dy)>, exact on integers
    assert (up * e.dy_up).sum() == (e.x * adj).sum()
    xr = T64(e.x).requires_grad_(True)
    ref = O.resize_bilinear(xr, 2 * h, 2 * w)
    (gx,) = torch.autograd.grad(ref, xr, T64(e.dy_up))
    assert torch.equal(ref.detach(), T64(up)) and torch.equal(gx, T64(adj))
    assert (e.mask == 0).mean() > 0.2 and (e.mask < 0).any()
    dz = adj * (e.mask > 0)
    assert np.abs(dz * e.mask).reshape(-1, c).sum(0).max() < 2 ** 24


# ---- bounded data: the f32 emulation ------------------------------------------------------------
def _emulate_forward(e):
    n = e.npix
    S = e.rows.astype(np.float64).sum(0)
    m = S[0] / n
    v = np.maximum(S[1] / n - m * m, 0.0)
    mean, var = F32(m), F32(v)
    rstd = F32(1.0 / np.sqrt(np.float64(var + R.EPS)))
    sc = F32(e.gamma) * rstd
    sh = F32(e.beta) - mean * sc
    out = np.maximum(F32(e.y) * sc + sh, F32(0))
    unb = v * n / (n - 1) if n > 1 else v
    om = F32(1) - R.MOMENTUM
    return dict(out=out, scale=sc, shift=sh, mean=mean, rstd=rstd, moving_mean=F32(e.mm) * R.MOMENTUM + mean * om,
                moving_var=F32(e.mv) * R.MOMENTUM + F32(unb) * om)


def _emulate_backward(e, relu):
    g, n, c = e.geo, e.npix, e.c
    y, d = F32(e.y), F32(e.dout)
    sc, sh, mu, rs = F32(e.scale), F32(e.shift), F32(e.mean), F32(e.rstd)
    v = y * sc + sh
    dz = np.where(v > 0, d, F32(0)) if relu else d
    xhat = (y - mu) * rs
    terms = np.stack([dz, dz * xhat], 1)                                      # [npix][2][c]
    part = np.zeros((g.nblk, 2, c), F32)
    for b in range(g.nblk):
        p0, p1 = b * g.per_blk, min((b + 1) * g.per_blk, n)
        lanes = np.zeros((g.rows, 2, c), F32)
        for t in range(g.trips):
            p = np.arange(p0 + t * g.rows, min(p0 + (t + 1) * g.rows, p1))
            if len(p):
                lanes[:len(p)] += terms[p]
        for r in range(g.rows):
            part[b] += lanes[r]
    S = part.astype(np.float64).sum(0)
    k0, k1, k2 = F32(e.gamma) * rs, F32(S[0] / n), F32(S[1] / n)
    return dict(s1=F32(S[0]), s2=F32(S[1]), dy=k0 * (dz - k1 - xhat * k2))


@pytest.mark.parametrize('c,npix,nrows', R.BOUNDED_SHAPES)
def test_emulation_stays_under_every_bound(c, npix, nrows):
    e = R.bounded_case(c, npix, nrows, torch.float32)
    b = R.forward_bounds(e.y, e.gamma, e.beta, e.st, e.mm, e.mv)
    got = _emulate_forward(e)
    rmm, rmv = R.moving(e.mm, e.mv, e.st)
    ref = dict(out=e.fwd.out, scale=e.fwd.scale, shift=e.fwd.shift, mean=e.st.mean, rstd=e.st.rstd, moving_mean=rmm, moving_var=rmv)
    for k in ref:
        assert not R.violations(got[k], ref[k], getattr(b, k)).any(), k
        print('EMU c%d n%d %s err/bound %.3f' % (c, npix, k, R.ratio(got[k], ref[k], getattr(b, k))))
    assert e.st.var[R.CH_CONST] == 0 and e.st.rstd[R.CH_CONST] == 1 / np.sqrt(float(R.EPS))
    for relu in (True, False):
        bb = R.backward_bounds(e.dout, e.y, e.scale, e.shift, e.mean, e.rstd, e.gamma, npix, e.geo.L, relu)
        got = _emulate_backward(e, relu)
        assert not R.violations(got['s1'], bb.ref.s1, bb.s1).any()
        assert not R.violations(got['s2'], bb.ref.s2, bb.s2).any()
        assert not (R.violations(got['dy'], bb.ref.dy, bb.dy) & ~bb.amb).any()
        print('EMU c%d n%d relu%d dy err/bound %.3f, left out %d' % (c, npix, relu, R.ratio(got['dy'][~bb.amb], bb.ref.dy[~bb.amb], bb.dy[~bb.amb]),
                                                                       bb.left_out))
        if relu:
            assert (bb.ref.dy[:, R.CH_DEAD] == 0).all() and bb.ref.s1[R.CH_DEAD] == 0 and bb.ref.s2[R.CH_DEAD] == 0
            assert (got['dy'][:, R.CH_DEAD] == 0).all()


@DT
@pytest.mark.parametrize('c,npix,nrows', R.BOUNDED_SHAPES)
def test_left_out_share(c, npix, nrows, dt):
    e = R.bounded_case(c, npix, nrows, dt)
    bb = R.backward_bounds(e.dout, e.y, e.scale, e.shift, e.mean, e.rstd, e.gamma, npix, e.geo.L)
    assert bb.left_out <= R.left_out_cap(npix, c), (bb.left_out, npix * c)


def test_one_pixel_case_needs_the_clamp():
    """(32, 1, 1) in f32 storage: the row holds f32(y^2), which is below y^2 in about half the channels, so S2/N - mean^2 < 0 there
    and only max(., 0) gives var == 0.  Without the clamp rstd leaves its 4 u bound in most of them: this is the case that holds the clamp (the
    constant channel and the integer tables have exact sums and never reach it)."""
    e = R.bounded_case(32, 1, 1, torch.float32)
    S = e.rows.astype(np.float64).sum(0)
    raw = S[1] - S[0] * S[0]
    assert (raw < 0).sum() >= 8 and (e.st.var[raw < 0] == 0).all()
    unclamped = 1.0 / np.sqrt(raw + float(R.EPS))
    b = R.forward_bounds(e.y, e.gamma, e.beta, e.st)
    assert R.violations(unclamped, e.st.rstd, b.rstd)[raw < 0].sum() >= 8          # (two of the sixteen have a tiny y)


def test_launch_geometry_restated():
    """col_reduce_blocks: 4 pixels per lane, at most 256 rows up to 4 M elements, 1024 above."""
    assert R.bwd_geometry(32776, 256).nblk == 1024 and R.bwd_geometry(1000, 64).nblk == 8 and R.bwd_geometry(1, 8).nblk == 1
    assert R.bwd_geometry(64, 2048).rows == 1 and R.bwd_geometry(1000, 8).rows == 256
    g = R.bwd_geometry(4096, 128)
    assert (g.nblk, g.rows, g.trips, g.L) == (64, 16, 4, 20)
