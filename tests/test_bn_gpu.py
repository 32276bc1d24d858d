"""The batch-norm kernels of imm_amd/csrc/elementwise.hip, each storage type (bf16, f16, f32), on a real MI355X.

1. Exact arithmetic, compared bit for bit: integers and dyadic constants (tests/bn_reference.py: exact_case, table, fused_table,
   exact_up), so that every result is independent of the summation order and of multiply-add contraction.  A 16-bit output is the
   one RNE of the exact value, an f32 output and every sum the exact value.  Pixels sit exactly on the ReLU edge y sc + sh == 0;
   gamma has a negative and a zero channel; the row counts of the finalize kernels cross every loop threshold of
   reduce_partials_32x32 (CPB 32: 64 row lanes; CPB 8 from 1024 rows: 256 row lanes; the scalar path at c % 4 != 0) and of
   slice32_reduce (16 row lanes: 128 rows per trip, 32 per trip, a tail).
2. Real data against the numpy f64 restatement within a-priori rounding bounds (the table in bn_reference's docstring): channels
   with mean/deviation 0.25, 8 and 64, a constant channel (var == 0), a channel dead behind the ReLU (dy, dgamma, dbeta exactly 0), a
   negative and a zero gamma, one pixel per channel; and the one chain in which E[x^2] - E[x]^2 is taken from sums a convolution's
   epilogue produced.  Each bounded test prints its largest err/bound and what it left out (run with -s).

Every device tensor is a guarded buffer (tests/guarded.py): an unwritten element is NaN, a stray store lands in a band.  What the
data must satisfy for all this to mean anything is asserted without a GPU in tests/test_bn_cpu.py.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import imm_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded                                                              # noqa: E402
from guarded import untouched                                               # noqa: E402
import bn_reference as R                                                    # noqa: E402
from exact_data import exact_equal                                          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
F32 = torch.float32
DT = pytest.mark.parametrize('dt', R.STORAGE, ids=R.STORAGE_IDS)
EPS, MOM = float(R.EPS), float(R.MOMENTUM)
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
    """The cached cases (up to 32 776 x 256 f64 values each) are dropped when the module is done."""
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


def wide(t, ld):
    """A kernel INPUT [..., c] embedded in [..., ld] on the device; the columns [c, ld) hold NaN."""
    c = t.shape[-1]
    o = torch.full(tuple(t.shape[:-1]) + (ld,), NAN, dtype=t.dtype)
    o[..., :c] = t
    return guarded.inp(o, DEV, depth=2)


def put(v64, dt, ld=None):
    """Exact f64 data as a guarded operand of type dt (asserted representable), rows `ld` wide when given."""
    t = R.store(v64, dt)
    assert torch.equal(t.double(), T64(v64)), 'not representable in %s' % dt
    return guarded.inp(t, DEV, depth=2) if ld is None else wide(t, ld)


def chan(v64):
    """A per-channel f32 array the kernels are handed (exact where the data are dyadic)."""
    return guarded.inp(torch.from_numpy(R.f32(v64)), DEV, depth=2)


def gout(shape, dt, fill=None):
    return guarded.out(shape, dt, DEV, fill=fill, what=guarded._caller(1))


def vec(n, fill=None):
    return guarded.out((n,), F32, DEV, fill=fill, what=guarded._caller(1))


def same(got, v64, dt, what):
    """got holds, bit for bit, what a kernel stores for v64: the nearest f32 value, rounded once more (RNE) to a 16-bit dt."""
    want = R.stored_bits(v64, dt)
    exact_equal(got, want, what, exact=T64(v64) if want.dtype == torch.int16 else None)


def totals(part, s1, s2, what):
    """The partial rows [nblk][2][c], every one finite, sum (f64, on the host) to the exact (s1, s2)."""
    assert bool(torch.isfinite(part).all()), '%s: a partial row is not finite' % what
    s = part.double().sum(0).cpu() + 0.0
    exact_equal(s[0], T64(s1) + 0.0, what + ': sum dz')
    exact_equal(s[1], T64(s2) + 0.0, what + ': second sum')


def held(got, ref, bound, dt, what, keep=None):
    """No element outside its bound (bn_reference.violations); returns err/bound for the report."""
    got = R.widen(got)
    bad = R.violations(got, ref, bound, dt)
    if keep is not None:
        bad &= keep
        got, ref, bound = got[keep], np.asarray(ref)[keep], np.asarray(bound)[keep]
    r = R.ratio(got, ref, bound, dt)
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError('%s: %d/%d elements outside their bound (%d not finite), largest err/bound %.3g, first at %s' % (
            what, int(bad.sum()), bad.size, int((~np.isfinite(got)).sum()), r, i))
    return r


# ==============================================================================================
# 1. exact arithmetic
# ==============================================================================================
@DT
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
@pytest.mark.parametrize('c,npix', R.APPLY_SHAPES)
def test_bn_apply_exact(ops, c, npix, relu, dt):
    e = R.exact_case(c, npix, R.Y_AMP[dt])
    ldy, ldx = c + 8, c + 16
    xo = gout((npix, ldx), dt)
    ops.bn_apply_relu(put(e.y, dt, ldy), npix, c, ldy, chan(e.scale), chan(e.shift), relu, xo, ldx)
    torch.cuda.synchronize()
    v = e.y * e.scale + e.shift
    same(xo[:, :c], np.maximum(v, 0.0) if relu else v, dt, 'bn_apply c%d' % c)
    assert untouched(xo[:, c:]), 'imm_bn_apply_relu wrote columns [c, ldx)'


@DT
@pytest.mark.parametrize('c,npix', R.REDUCE_SHAPES)
def test_bn_bwd_reduce_exact(ops, c, npix, dt):
    e = R.exact_case(c, npix)
    geo = R.bwd_geometry(npix, c)
    nblk = ops.bn_bwd_blocks(npix, c)
    assert nblk == geo.nblk
    if (c, npix) == (256, 32776):
        assert nblk == 1024, 'this case must reach the cap on the partial rows'
    lddo, ldy = c + 16, c + 8
    dow, yw = put(e.dout, dt, lddo), put(e.y, dt, ldy)
    consts = [chan(a) for a in (e.scale, e.shift, e.mean, e.rstd)]
    for relu in (True, False):
        part = gout((nblk, 2, c), F32)
        ops.bn_bwd_reduce(dow, lddo, yw, ldy, npix, c, *consts, relu, part)
        torch.cuda.synchronize()
        r = R.backward(e.dout, e.y, e.scale, e.shift, e.mean, e.rstd, e.gamma, npix, relu)
        totals(part, r.s1, r.s2, 'bn_bwd_reduce c%d relu%d' % (c, relu))


@DT
@pytest.mark.parametrize('B,h,w,c', R.UP_SHAPES)
def test_bn_bwd_reduce_up_exact(ops, B, h, w, c, dt):
    e = R.exact_up(B, h, w, c)
    npix = B * h * w
    nblk = ops.bn_bwd_blocks(npix, c)
    lddy, lddp, ldy = c + 8, c + 16, c + 24
    dprev = gout((B, h, w, lddp), dt)
    part = gout((nblk, 2, c), F32)
    ops.bn_bwd_reduce_up(put(e.dy_up, dt, lddy), lddy, dprev, lddp, put(e.y, dt, ldy), ldy, B, h, w, c,
                         chan(e.scale), chan(e.shift), chan(e.mean), chan(e.rstd), True, part)
    torch.cuda.synchronize()
    adj = R.up_bwd(e.dy_up)
    same(dprev[..., :c], adj, dt, 'bn_bwd_reduce_up/dprev')
    assert untouched(dprev[..., c:])
    r = R.backward(adj.reshape(npix, c), e.y.reshape(npix, c), e.scale, e.shift, e.mean, e.rstd, e.gamma, npix)
    totals(part, r.s1, r.s2, 'bn_bwd_reduce_up')


@DT
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
@pytest.mark.parametrize('c,npix', R.APPLY_SHAPES)
def test_bn_bwd_apply_exact(ops, c, npix, relu, dt):
    e = R.exact_case(c, npix)
    lddo, ldy, lddy = c + 16, c + 8, c + 24
    dyo = gout((npix, lddy), dt)
    ops.bn_bwd_apply(put(e.dout, dt, lddo), lddo, put(e.y, dt, ldy), ldy, npix, c, chan(e.scale), chan(e.shift), chan(e.mean),
                     chan(e.rstd), relu, chan(e.coef), dyo, lddy)
    torch.cuda.synchronize()
    same(dyo[:, :c], R.apply_coef(e.dout, e.y, e.scale, e.shift, e.mean, e.rstd, e.coef, relu), dt, 'bn_bwd_apply c%d' % c)
    assert untouched(dyo[:, c:]), 'imm_bn_bwd_apply wrote columns [c, lddy)'


@pytest.mark.parametrize('from_out', [False, True], ids=['sums', 'from_out'])
@pytest.mark.parametrize('c,nblk', R.FINALIZE_CASES)
def test_bn_bwd_finalize_exact(ops, c, nblk, from_out):
    ldp, count = R.finalize_ldp(c), 1000
    t = R.table(nblk, c, ldp)
    ch = R.exact_channels(c, c)
    dg, db, coef = vec(c), vec(c), gout((3, c), F32)
    ops.bn_bwd_finalize(dev(torch.from_numpy(t)), nblk, c, count, chan(ch.gamma), chan(ch.beta), chan(ch.rstd), dg, db, coef,
                        from_out=from_out, ldp=ldp)
    torch.cuda.synchronize()
    S = t[:, :, :c].astype(np.float64).sum(0)
    s1, s2 = R.from_out(t[:, :, :c], ch.gamma, ch.beta) if from_out else (S[0], S[1])
    what = 'bn_bwd_finalize c%d nblk%d' % (c, nblk)
    same(db, s1, F32, what + '/dbeta')
    same(dg, s2, F32, what + '/dgamma')
    same(coef[0], ch.gamma * ch.rstd, F32, what + '/coef0')
    same(coef[1], s1 / count, F32, what + '/coef1')
    same(coef[2], s2 / count, F32, what + '/coef2')
    if from_out:
        assert s2[2] == 0 and ch.gamma[2] == 0                                # gamma == 0 -> 0, not a division


@pytest.mark.parametrize('c,nblk', R.FINALIZE_CASES)
def test_bn_finalize_on_integer_tables(ops, c, nblk):
    """The forward twin on the same tables: mean bit for bit, everything behind rsqrtf within the bounds of section 2."""
    count = nblk * 7
    t = np.ascontiguousarray(R.table(nblk, c, R.finalize_ldp(c))[:, :, :c])
    ch = R.exact_channels(c, c)
    mm0, mv0 = ch.mean / 4, ch.rstd
    mm, mv = vec(c, torch.from_numpy(R.f32(mm0))), vec(c, torch.from_numpy(R.f32(mv0)))
    scale, shift, mean, rstd = (vec(c) for _ in range(4))
    ops.bn_finalize(dev(torch.from_numpy(t)), nblk, c, count, chan(ch.gamma), chan(ch.beta), EPS, MOM, True, mm, mv, scale, shift, mean, rstd)
    torch.cuda.synchronize()
    st = R.stats(t, count)
    same(mean, st.mean, F32, 'bn_finalize c%d nblk%d/mean' % (c, nblk))
    b = R.forward_bounds(np.zeros((1, c)), ch.gamma, ch.beta, st, mm0, mv0)
    f = R.forward(np.zeros((1, c)), ch.gamma, ch.beta, st)
    rmm, rmv = R.moving(mm0, mv0, st)
    for got, ref, bound, what in ((rstd, st.rstd, b.rstd, 'rstd'), (scale, f.scale, b.scale, 'scale'), (shift, f.shift, b.shift, 'shift'),
                                  (mm, rmm, b.moving_mean, 'moving_mean'), (mv, rmv, b.moving_var, 'moving_var')):
        held(got, ref, bound, F32, 'bn_finalize c%d nblk%d/%s' % (c, nblk, what))


@DT
@pytest.mark.parametrize('c,count,nblk', R.FUSED_CASES)
def test_bn_bwd_apply_fused_exact(ops, c, count, nblk, dt):
    e = R.exact_case(c, count)
    tab = R.fused_table(nblk, c)
    lddo, ldy, lddy = c + 16, c + 8, c + 24
    dg, db, dyo = vec(c), vec(c), gout((count, lddy), dt)
    ops.bn_bwd_apply_fused(dev(torch.from_numpy(tab)), nblk, c, count, chan(e.gamma), put(e.dout, dt, lddo), lddo, put(e.y, dt, ldy), ldy,
                           chan(e.scale), chan(e.shift), chan(e.mean), chan(e.rstd), True, dg, db, dyo, lddy)
    torch.cuda.synchronize()
    S = tab.astype(np.float64).sum(0)
    what = 'bn_bwd_apply_fused c%d n%d nblk%d' % (c, count, nblk)
    same(db, S[0], F32, what + '/dbeta')
    same(dg, S[1], F32, what + '/dgamma')
    coef = np.stack([e.gamma * e.rstd, S[0] / count, S[1] / count])
    same(dyo[:, :c], R.apply_coef(e.dout, e.y, e.scale, e.shift, e.mean, e.rstd, coef), dt, what + '/dy')
    assert untouched(dyo[:, c:]), 'imm_bn_bwd_apply_fused wrote columns [c, lddy)'


@pytest.mark.parametrize('rows,width,group', R.ROWS_REDUCE)
def test_rows_reduce_exact(ops, rows, width, group):
    g = np.random.RandomState(rows + width)
    src = g.randint(-1000, 1001, size=(rows, width)).astype(np.float64)
    n = -(-rows // group)
    dst = gout((n, width), F32)
    ops.rows_reduce(put(src, F32), rows, width, group, dst)
    torch.cuda.synchronize()
    pad = np.zeros((n * group, width))
    pad[:rows] = src
    same(dst, pad.reshape(n, group, width).sum(1), F32, 'rows_reduce')


@DT
@pytest.mark.parametrize('B,h,w,c', R.UP_SHAPES)
def test_upsample2x_exact(ops, B, h, w, c, dt):
    e = R.exact_up(B, h, w, c)
    lds, ldu, ldo = c + 8, c + 16, c + 24
    up = gout((B, 2 * h, 2 * w, ldu), dt)
    ops.upsample2x_fwd(put(e.x, dt, lds), up, B, h, w, c, lds, ldu)
    dyw = put(e.dy_up, dt, ldu)
    dx = gout((B, h, w, lds), dt)
    ops.upsample2x_bwd(dyw, dx, B, h, w, c, ldu, lds)
    nblk = ops.upsample2x_bwd_bn_blocks(B, h, w, c)
    part = gout((nblk, 2, c), F32)
    dxm = gout((B, h, w, lds), dt)
    ops.upsample2x_bwd_bn(dyw, dxm, B, h, w, c, ldu, lds, put(e.mask, dt, ldo), ldo, part)
    torch.cuda.synchronize()
    adj = R.up_bwd(e.dy_up)
    same(up[..., :c], R.up_fwd(e.x), dt, 'upsample2x_fwd')
    same(dx[..., :c], adj, dt, 'upsample2x_bwd')
    dz = np.where(e.mask > 0, adj, 0.0)
    same(dxm[..., :c], dz, dt, 'upsample2x_bwd_bn/dx')
    totals(part, dz.reshape(-1, c).sum(0), (dz * e.mask).reshape(-1, c).sum(0), 'upsample2x_bwd_bn')
    assert untouched(up[..., c:]) and untouched(dx[..., c:]) and untouched(dxm[..., c:])


@DT
@pytest.mark.parametrize('c,npix', R.COLSUM_SHAPES)
def test_colsum_exact_at_the_edges(ops, c, npix, dt):
    x = np.random.RandomState(c + npix).randint(-8, 9, size=(npix, c)).astype(np.float64)
    ld = c + 8
    part = gout((ops.colsum_blocks(npix, c), c), F32)
    out = vec(c)
    ops.colsum(put(x, dt, ld), npix, c, c, ld, part, out)
    torch.cuda.synchronize()
    same(out, x.sum(0), F32, 'colsum c%d npix%d' % (c, npix))


# ==============================================================================================
# 2. real data, held to the f64 reference within the derived bounds
# ==============================================================================================
BOUNDED = pytest.mark.parametrize('c,npix,nrows', R.BOUNDED_SHAPES)
PATH = pytest.mark.parametrize('fused', [False, True], ids=['pair', 'fused'])


def _forward(ops, e, fused, training, mm, mv, rows, nrows):
    c, npix = e.c, e.npix
    ldy, ldx = c + 8, c + 16
    scale, shift, mean, rstd = (vec(c) for _ in range(4))
    xo = gout((npix, ldx), e.dt)
    yw, g, b = wide(e.y_t, ldy), chan(e.gamma), chan(e.beta)
    if fused:
        ops.bn_apply_fused(rows, nrows, c, npix, g, b, EPS, MOM, training, mm, mv, scale, shift, mean, rstd, yw, ldy, True, xo, ldx)
    else:
        ops.bn_finalize(rows, nrows, c, npix, g, b, EPS, MOM, training, mm, mv, scale, shift, mean, rstd)
        ops.bn_apply_relu(yw, npix, c, ldy, scale, shift, True, xo, ldx)
    torch.cuda.synchronize()
    assert untouched(xo[:, c:]), 'columns [c, ldx) of the output were written'
    return dict(out=xo[:, :c], scale=scale, shift=shift, mean=mean, rstd=rstd)


@DT
@PATH
@BOUNDED
def test_bn_forward_training_bounded(ops, c, npix, nrows, fused, dt):
    e = R.bounded_case(c, npix, nrows, dt)
    mm, mv = vec(c, torch.from_numpy(R.f32(e.mm))), vec(c, torch.from_numpy(R.f32(e.mv)))
    got = _forward(ops, e, fused, True, mm, mv, dev(torch.from_numpy(e.rows)), nrows)
    got.update(moving_mean=mm, moving_var=mv)
    b = R.forward_bounds(e.y, e.gamma, e.beta, e.st, e.mm, e.mv)
    rmm, rmv = R.moving(e.mm, e.mv, e.st)
    ref = dict(out=e.fwd.out, scale=e.fwd.scale, shift=e.fwd.shift, mean=e.st.mean, rstd=e.st.rstd, moving_mean=rmm, moving_var=rmv)
    rep = {k: held(got[k], ref[k], getattr(b, k), dt if k == 'out' else F32, 'bn forward/' + k) for k in ref}
    print('BN_FWD c%d n%d %s %s err/bound: %s' % (c, npix, 'fused' if fused else 'pair', str(dt)[6:],
                                                    ' '.join('%s %.3f' % kv for kv in rep.items())))
    assert e.st.var[R.CH_CONST] == 0, 'the constant channel has exact sums'
    assert float(got['out'][:, R.CH_DEAD].float().abs().max()) == 0.0, 'the dead channel stores zeros'


@DT
@PATH
@BOUNDED
def test_bn_forward_eval_bounded(ops, c, npix, nrows, fused, dt):
    e = R.bounded_case(c, npix, nrows, dt)
    mm0, mv0 = torch.from_numpy(R.f32(e.mm)), torch.from_numpy(R.f32(e.mv))
    mm, mv = vec(c, mm0), vec(c, mv0)
    got = _forward(ops, e, fused, False, mm, mv, None, 0)
    st = R.eval_stats(e.mm, e.mv)
    f = R.forward(e.y, e.gamma, e.beta, st)
    b = R.forward_bounds(e.y, e.gamma, e.beta, st)
    ref = dict(out=f.out, scale=f.scale, shift=f.shift, mean=st.mean, rstd=st.rstd)
    rep = {k: held(got[k], ref[k], getattr(b, k), dt if k == 'out' else F32, 'bn eval/' + k) for k in ref}
    print('BN_EVAL c%d n%d %s %s err/bound: %s' % (c, npix, 'fused' if fused else 'pair', str(dt)[6:],
                                                     ' '.join('%s %.3f' % kv for kv in rep.items())))
    exact_equal(mm, mm0, 'eval mode must leave moving_mean untouched')
    exact_equal(mv, mv0, 'eval mode must leave moving_var untouched')


@DT
@PATH
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
@BOUNDED
def test_bn_backward_bounded(ops, c, npix, nrows, relu, fused, dt):
    e = R.bounded_case(c, npix, nrows, dt)
    bb = R.cached(('bwd_bounds', c, npix, nrows, dt, relu),
                  lambda: R.backward_bounds(e.dout, e.y, e.scale, e.shift, e.mean, e.rstd, e.gamma, npix, e.geo.L, relu))
    assert bb.left_out <= R.left_out_cap(npix, c)
    nblk = ops.bn_bwd_blocks(npix, c)
    assert nblk == e.geo.nblk
    lddo, ldy, lddy = c + 16, c + 8, c + 24
    dow, yw = wide(e.dout_t, lddo), wide(e.y_t, ldy)
    g, consts = chan(e.gamma), [chan(a) for a in (e.scale, e.shift, e.mean, e.rstd)]
    part = gout((nblk, 2, c), F32)
    ops.bn_bwd_reduce(dow, lddo, yw, ldy, npix, c, *consts, relu, part)
    dg, db, dyo = vec(c), vec(c), gout((npix, lddy), dt)
    if fused:
        ops.bn_bwd_apply_fused(part, nblk, c, npix, g, dow, lddo, yw, ldy, *consts, relu, dg, db, dyo, lddy)
    else:
        coef = gout((3, c), F32)
        ops.bn_bwd_finalize(part, nblk, c, npix, g, chan(e.beta), consts[3], dg, db, coef)
        ops.bn_bwd_apply(dow, lddo, yw, ldy, npix, c, *consts, relu, coef, dyo, lddy)
    torch.cuda.synchronize()
    r = bb.ref
    rep = (held(db, r.s1, bb.s1, F32, 'dbeta'), held(dg, r.s2, bb.s2, F32, 'dgamma'),
           held(dyo[:, :c], r.dy, bb.dy, dt, 'dy', keep=~bb.amb))
    print('BN_BWD c%d n%d %s %s %s err/bound: dbeta %.3f dgamma %.3f dy %.3f, left out %d of %d' % (
        (c, npix, 'relu' if relu else 'linear', 'fused' if fused else 'pair', str(dt)[6:]) + rep + (bb.left_out, npix * c)))
    assert untouched(dyo[:, c:]), 'columns [c, lddy) of dy were written'
    assert float(dyo[:, R.CH_ZERO].float().abs().max()) == 0.0, 'gamma == 0: dy is zero'
    if relu:
        assert float(dyo[:, R.CH_DEAD].float().abs().max()) == 0.0 and float(dg[R.CH_DEAD]) == 0.0 and float(db[R.CH_DEAD]) == 0.0, \
            'the channel dead behind the ReLU has dy, dgamma and dbeta exactly 0'


@pytest.mark.parametrize('dt', R.STORAGE[:2], ids=R.STORAGE_IDS[:2])
def test_bn_statistics_from_the_real_producer(ops, dt):
    """A 3x3 convolution with IMM_CONV_STATS -> (imm_rows_reduce above 256 rows, as the engine does) -> imm_bn_apply_fused, with a
    bias that puts mean/deviation near 16: the one place where the cancellation of E[x^2] - E[x]^2 is measured from end to end.
    mean and var of the kernel's rows against a two-pass f64 variance of the f64 convolution of the same 16-bit inputs:
        |var - ref| <= (n + 2) u (1 + (mean/dev)^2) ref,   |mean - ref| <= (n + 2) u mean|v|,   n = pixels per partial row
    (a sum of n f32 terms and the product v * v; S2/N - mean^2 amplifies the relative error of S2/N by 1 + (mean/dev)^2).
    MEASURED on an MI355X (32 rows of 64 pixels): relative variance error 9.8e-6 (bf16), 1.0e-5 (f16) against a bound of 1.01e-3; the
    mean at 0.005 of its bound."""
    from imm_amd import _lib as L
    from test_kernels_gpu import run_conv
    B, H, ci, co = 2, 32, 32, 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, H, H, ci, generator=g).to(dt)
    w = (torch.randn(3, 3, ci, co, generator=g) * 0.1).to(dt)
    v0 = O.conv2d_same(x.double(), w.double(), None, 1).reshape(-1, co)
    bias = (16.0 * v0.std(0)).float()
    v = (v0 + bias.double()).numpy()
    mean_ref = v.mean(0)
    var_ref = ((v - mean_ref) ** 2).mean(0)
    y, stats, desc = run_conv(ops, x, w, bias, 3, 1, co, ci, False, extra_flags=L.CONV_STATS)
    npix = B * H * H
    nb = ops.conv_stats_blocks(desc)
    n = -(-npix // nb)
    rows, nrows = stats, nb
    if nb > 256:                                          # idle at this shape (32 rows): the engine's rule, kept for a dispatch that splits finer;
                                                          # imm_rows_reduce itself is covered by test_rows_reduce_exact
        nrows = -(-nb // 32)
        rows = gout((nrows, 2, co), F32)
        ops.rows_reduce(stats, nb, 2 * co, 32, rows)
    gamma, beta = 1.0 + 0.25 * np.cos(np.arange(co)), 0.5 * np.sin(np.arange(co))
    mm, mv = vec(co, 0.0), vec(co, 1.0)
    scale, shift, mean, rstd = (vec(co) for _ in range(4))
    ldy = y.shape[-1]
    xo = gout((npix, co), dt)
    ops.bn_apply_fused(rows, nrows, co, npix, chan(gamma), chan(beta), EPS, MOM, True, mm, mv, scale, shift, mean, rstd, y, ldy, True, xo, co)
    torch.cuda.synchronize()
    # the statistics the kernel's own rows hold, against the two-pass reference
    S = stats.double().sum(0).cpu().numpy()
    mean_k = S[0] / npix
    var_k = S[1] / npix - mean_k ** 2
    ratio2 = 1.0 + mean_ref ** 2 / var_ref
    var_bound = (n + 2) * R.U * ratio2
    var_err = np.abs(var_k - var_ref) / var_ref
    mean_bound = (n + 2) * R.U * np.abs(v).mean(0)
    print('BN_PRODUCER %s: %d rows of %d pixels, mean/dev %.1f..%.1f, max rel var err %.3g (bound %.3g, err/bound %.3f), max mean err/bound %.3f' % (
        str(dt)[6:], nb, n, np.sqrt(ratio2.min() - 1), np.sqrt(ratio2.max() - 1), var_err.max(), var_bound[var_err.argmax()],
        (var_err / var_bound).max(), (np.abs(mean_k - mean_ref) / mean_bound).max()))
    assert 12 < np.sqrt(ratio2.min() - 1) and np.sqrt(ratio2.max() - 1) < 20
    assert (np.abs(mean_k - mean_ref) <= mean_bound).all()
    assert (var_err <= var_bound).all(), (var_err / var_bound).max()
    # and the pass that consumes them, against the reference on those rows
    rows_h = rows.cpu().numpy()
    st = R.stats(rows_h, npix)
    yv = R.widen(y.reshape(npix, ldy)[:, :co])
    gamma_f, beta_f = R.f32(gamma).astype(np.float64), R.f32(beta).astype(np.float64)
    f = R.forward(yv, gamma_f, beta_f, st)
    b = R.forward_bounds(yv, gamma_f, beta_f, st, np.zeros(co), np.ones(co))
    rmm, rmv = R.moving(np.zeros(co), np.ones(co), st)
    for got, ref, bound, sdt, what in ((xo, f.out, b.out, dt, 'out'), (mean, st.mean, b.mean, F32, 'mean'), (rstd, st.rstd, b.rstd, F32, 'rstd'),
                                       (scale, f.scale, b.scale, F32, 'scale'), (shift, f.shift, b.shift, F32, 'shift'),
                                       (mm, rmm, b.moving_mean, F32, 'moving_mean'), (mv, rmv, b.moving_var, F32, 'moving_var')):
        held(got, ref, bound, sdt, 'producer chain/' + what)
    # rstd against the two-pass variance: half the relative error of var (+ the 4 u of the rstd chain)
    held(rstd, 1 / np.sqrt(var_ref + EPS), (0.5 * var_bound + 4 * R.U) / np.sqrt(var_ref + EPS), F32, 'producer chain/rstd vs two-pass')


# ---- the fused paths in f32 storage: the three bit-for-bit equalities of the 16-bit suites, at their smallest shapes ----------
def _randn(shape, seed, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


def test_f32_bn_apply_fused_upsampling_equals_upsample2x_fwd(ops):
    B, h, w, c, ldy, ldo, ldu = 2, 8, 8, 32, 32, 40, 32
    npix = B * h * w
    y = _randn((npix, c), 241, 2.0, 0.5)
    gamma, beta = dev(_randn((c,), 242, 0.5, 1.0)), dev(_randn((c,), 243, 0.5))
    mm, mv = dev(_randn((c,), 244, 0.3, 0.5)), dev(_randn((c,), 245, 0.2).abs() + 1.0)
    s2, h2, m2, r2 = (vec(c) for _ in range(4))
    yw = wide(y, ldy)
    xo, up = gout((npix, ldo), F32), gout((B, 2 * h, 2 * w, ldu), F32)
    ops.bn_apply_fused(None, 0, c, npix, gamma, beta, EPS, MOM, False, mm, mv, s2, h2, m2, r2, yw, ldy, True, xo, ldo, up, ldu, h, w)
    xp = gout((npix, ldo), F32)
    ops.bn_apply_fused(None, 0, c, npix, gamma, beta, EPS, MOM, False, mm, mv, s2, h2, m2, r2, yw, ldy, True, xp, ldo)
    up_r = gout((B, 2 * h, 2 * w, c), F32)
    ops.upsample2x_fwd(dev(xo[:, :c].contiguous()).reshape(B, h, w, c), up_r, B, h, w, c, c, c)
    torch.cuda.synchronize()
    assert torch.equal(xo[:, :c], xp[:, :c]) and bool(torch.isfinite(xo[:, :c]).all())
    assert torch.equal(up[..., :c], up_r), 'the fused up-sampled output differs from imm_upsample2x_fwd of the stored tensor'
    assert untouched(xo[:, c:]) and untouched(up[..., c:])


def test_f32_bn_bwd_reduce_up_equals_the_two_launches(ops):
    B, h, c = 2, 8, 16
    npix = B * h * h
    dy_up, y = dev(_randn((B, 2 * h, 2 * h, c), 191)), dev(_randn((B, h, h, c), 192, 2.0, 0.3))
    scale, shift = dev(_randn((c,), 193, 0.3, 1.0)), dev(_randn((c,), 194, 0.5))
    mean, rstd = dev(_randn((c,), 195, 0.5)), dev(_randn((c,), 196, 0.1).abs() + 0.5)
    nblk = ops.bn_bwd_blocks(npix, c)
    d_ref, p_ref = gout((B, h, h, c), F32), gout((nblk, 2, c), F32)
    ops.upsample2x_bwd(dy_up, d_ref, B, h, h, c, c, c)
    ops.bn_bwd_reduce(d_ref, c, y, c, npix, c, scale, shift, mean, rstd, True, p_ref)
    d_got, p_got = gout((B, h, h, c), F32), gout((nblk, 2, c), F32)
    ops.bn_bwd_reduce_up(dy_up, c, d_got, c, y, c, B, h, h, c, scale, shift, mean, rstd, True, p_got)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(d_ref).all()) and torch.equal(d_got, d_ref)
    assert torch.equal(p_got, p_ref), float((p_got - p_ref).abs().max())


def test_f32_upsample2x_bwd_bn_equals_upsample2x_bwd(ops):
    B, h, c = 2, 8, 16
    dy, out = dev(_randn((B, 2 * h, 2 * h, c), 52)), dev(_randn((B, h, h, c), 55))
    plain = gout((B, h, h, c), F32)
    ops.upsample2x_bwd(dy, plain, B, h, h, c, c, c)
    nblk = ops.upsample2x_bwd_bn_blocks(B, h, h, c)
    part, dx = gout((nblk, 2, c), F32), gout((B, h, h, c), F32)
    ops.upsample2x_bwd_bn(dy, dx, B, h, h, c, c, c, out, c, part)
    torch.cuda.synchronize()
    want = plain * (out > 0)
    assert bool(torch.isfinite(plain).all()) and torch.equal(dx, want)
    # sums of at most B h h f32 terms each (+ the product): (n + 1) u sum|terms|
    wd, od = R.widen(want).reshape(-1, c), R.widen(out).reshape(-1, c)
    n = B * h * h
    s = R.widen(part).sum(0)
    held(T64(s[0]), wd.sum(0), (n + 1) * R.U * np.abs(wd).sum(0), F32, 'upsample2x_bwd_bn f32/sum dz')
    held(T64(s[1]), (wd * od).sum(0), (n + 1) * R.U * np.abs(wd * od).sum(0), F32, 'upsample2x_bwd_bn f32/sum dz*out')
