"""Batch norm as imm_amd/csrc/elementwise.hip states it, in numpy f64, with a-priori rounding bounds and the data of
tests/test_bn_cpu.py and tests/test_bn_gpu.py.  No torch autograd, no GPU; torch is used only to round to bf16 / f16.

The rule (N = pixels per channel, rows = the f32 partial sums (sum y, sum y^2) the producer of y left):
    mean = S1/N   var = max(S2/N - mean^2, 0)   unbiased = var N/(N-1) (N > 1)   rstd = 1/sqrt(var + eps)
    sc = gamma rstd   sh = beta - mean sc   out = relu(y sc + sh)
    moving_mean = moving_mean m + mean (1 - m)        moving_var = moving_var m + unbiased (1 - m)
    dz = dout [y sc + sh > 0]   xhat = (y - mean) rstd   s1 = sum dz (= dbeta)   s2 = sum dz xhat (= dgamma)
    dy = gamma rstd (dz - s1/N - xhat s2/N)
    from the stored activation out = relu(gamma xhat + beta):  s2 = (sum dz out - beta s1)/gamma, 0 where gamma == 0

Bounds.  u = 2^-24 (half an ulp of f32, relative).  Each constant is the number of f32 roundings on the longest chain to the
quantity, times the magnitude each acts on; f64 steps of the kernels (the sums over the partial rows, S/N, S2/N - mean^2) count 0.

    mean          1   the cast of S1/N
    rstd          4   rsqrtf taken as good to 2 ulp = 4 u: the cast of var (1/2) and var + eps (1/2) fit inside the 4 only if it is good
                  to 1.5 ulp.  rstd is an output, so every run asserts the 4 on it directly; measured on an MI355X the largest error
                  of the whole chain is 1.8 u (0.45 of the bound), i.e. rsqrtf within 1 ulp on these inputs
    scale         5   rstd (4), gamma * rstd (1)
    shift         8 on |mean sc|: mean (1), sc (5), mean * sc (1), the subtraction (1);  1 on |beta|: the subtraction
    out           8 on |y sc| + |mean sc| + |beta|: sc (5) acts on (y - mean) sc, the cast of mean (1) and mean * sc (1) on |mean sc|,
                  y * sc (1) on |y sc|, the subtraction on |beta| + |mean sc|, the last addition on their sum: 8 on |y sc|; the
                  worst case on |mean sc| alone is 9, which no data reaches (the f32 emulation peaks at 0.34 of the bound)
    moving_*      2 on |old m|: product, sum;  3 on |new (1 - m)|: cast of mean / unbiased, product, sum  (1 - m is exact: m >= 1/2)
    s1 (dbeta)    L on sum|dz|: L = trips of a lane + pixel rows of a workgroup = the additions of the longest chain + 2, the 2
                  being the first addition of each chain (to zero: exact), which stand for the cast of the f64 total
    s2 (dgamma)   L on sum|dz xhat| (the 2 spare: dz * xhat and the cast), and sum |dz| e: xhat is wrong by e u with
                  e = 3 (|y| + |mean|) rstd: the subtraction (1) and the product (1) act on at most (|y| + |mean|) rstd; 1 spare
    dy            |gamma rstd| u (4 (|dz| + |k1| + |xhat k2|) + L A1 + |xhat| (L A2 + E) + e |k2|):  4 = gamma * rstd (1), the cast of
                  k (1) or xhat * k2 (1), the subtractions (1 each, on at most the sum), the last product (1);  A1 = sum|dz|/N and
                  A2 = sum|dz xhat|/N, E = sum|dz| e / N carry the error of the sums into k1 and k2
    16-bit store  + half an ulp of the stored type at |ref| + bound

The ReLU decision y sc + sh > 0 is taken in f32 from the f32 sc and sh the kernel is handed; where |y sc + sh| <= 4 u (|y sc| + |sh|)
(product, sum, and as much again to spare) f32 and f64 may disagree.  Those pixels are left out of the dy comparison and counted
(at most 0.1 % of a case), and what they can move the sums by (sum |dout|, sum |dout xhat| over them) is added to the bounds of s1,
s2 and dy.  relu() is continuous, so the forward comparison leaves nothing out.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from exact_data import rne16

U = 2.0 ** -24
EPS = np.float32(1e-3)
MOMENTUM = np.float32(0.99)
F64 = np.float64
STORAGE = [torch.bfloat16, torch.float16, torch.float32]
STORAGE_IDS = ['bf16', 'f16', 'f32']
_P = {torch.bfloat16: (8, -126), torch.float16: (11, -14)}        # significant bits, exponent of the smallest normal


def store(v64, dt):
    """f64 numpy -> the tensor of type dt a kernel would read (one rounding, none for data made representable)."""
    return torch.from_numpy(np.ascontiguousarray(v64, dtype=F64)).float().to(dt)


def widen(t):
    return t.detach().cpu().to(torch.float64).numpy()


def f32(v):
    return np.asarray(v, dtype=F64).astype(np.float32)


# ----------------------------------------------------------------------------------------------
# the rule
# ----------------------------------------------------------------------------------------------
def stats(rows_f32, count, eps_f32=EPS):
    rows = np.asarray(rows_f32)
    assert rows.dtype == np.float32 and rows.ndim == 3 and rows.shape[1] == 2, (rows.dtype, rows.shape)
    S = rows.astype(F64).sum(0)
    mean = S[0] / count
    var = np.maximum(S[1] / count - mean * mean, 0.0)
    unbiased = var * count / (count - 1.0) if count > 1 else var
    return SimpleNamespace(mean=mean, var=var, unbiased=unbiased, rstd=1.0 / np.sqrt(var + float(np.float32(eps_f32))), count=count)


def eval_stats(moving_mean_f32, moving_var_f32, eps_f32=EPS):
    mean, var = np.asarray(moving_mean_f32, F64), np.asarray(moving_var_f32, F64)
    return SimpleNamespace(mean=mean, var=var, unbiased=var, rstd=1.0 / np.sqrt(var + float(np.float32(eps_f32))), count=0)


def forward(y, gamma, beta, st, relu=True):
    sc = gamma * st.rstd
    sh = beta - st.mean * sc
    v = y * sc + sh
    return SimpleNamespace(out=np.maximum(v, 0.0) if relu else v, v=v, scale=sc, shift=sh)


def moving(mm, mv, st, momentum=MOMENTUM):
    m = float(np.float32(momentum))
    return mm * m + st.mean * (1.0 - m), mv * m + st.unbiased * (1.0 - m)


def backward(dout, y, scale, shift, mean, rstd, gamma, count, relu=True):
    v = y * scale + shift
    dz = np.where(v > 0, dout, 0.0) if relu else dout                        # (not dout * mask: that leaves -0.0)
    xhat = (y - mean) * rstd
    s1, s2 = dz.sum(0), (dz * xhat).sum(0)
    coef = np.stack([gamma * rstd, s1 / count, s2 / count])
    return SimpleNamespace(dz=dz, xhat=xhat, v=v, s1=s1, s2=s2, coef=coef, dy=coef[0] * (dz - coef[1] - xhat * coef[2]))


def apply_coef(dout, y, scale, shift, mean, rstd, coef, relu=True):
    """imm_bn_bwd_apply with a given coef table."""
    dz = np.where(y * scale + shift > 0, dout, 0.0) if relu else dout
    return coef[0] * (dz - coef[1] - (y - mean) * rstd * coef[2])


def from_out(rows_f32, gamma, beta):
    S = np.asarray(rows_f32).astype(F64).sum(0)
    with np.errstate(divide='ignore', invalid='ignore'):
        s2 = np.where(gamma != 0, (S[1] - beta * S[0]) / gamma, 0.0)
    return S[0], s2


# ----------------------------------------------------------------------------------------------
# launch geometry of the column reductions (col_reduce_blocks), restated so that L is known before any GPU runs
# ----------------------------------------------------------------------------------------------
def bwd_geometry(npix, c):
    assert c % 8 == 0 and 256 % (c // 8) == 0
    rows = 256 // (c // 8)
    nblk = max(1, -(-npix // (rows * 4)))
    nblk = min(nblk, 256 if npix * c <= (1 << 22) else 1024)
    per_blk = -(-npix // nblk)
    return SimpleNamespace(nblk=nblk, rows=rows, per_blk=per_blk, trips=-(-per_blk // rows), L=-(-per_blk // rows) + rows)


# ----------------------------------------------------------------------------------------------
# bounds and the one comparison
# ----------------------------------------------------------------------------------------------
def half_ulp(x, dt):
    """Half an ulp of dt at magnitude x (0 for f32 storage: the f32 roundings are in the bound)."""
    if dt == torch.float32:
        return np.zeros_like(x)
    p, emin = _P[dt]
    e = np.floor(np.log2(np.maximum(x, 2.0 ** emin)))
    return 2.0 ** (e - p)


def violations(got, ref, bound, dt=torch.float32):
    """Elements with |got - ref| > bound (+ half an ulp of a 16-bit store); a NaN in got is a violation."""
    got, ref, bound = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(bound, F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(ref).all() and np.isfinite(bound).all(), 'the REFERENCE or its bound is not finite: a bug of the test'
    tol = bound + half_ulp(np.abs(ref) + bound, dt)
    return ~(np.abs(got - ref) <= tol)


def ratio(got, ref, bound, dt=torch.float32):
    """max err / (bound + half ulp) over the elements with a non-zero tolerance (what the tests print)."""
    got, ref, bound = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(bound, F64)
    tol = bound + half_ulp(np.abs(ref) + bound, dt)
    nz = tol > 0
    return float((np.abs(got - ref)[nz] / tol[nz]).max()) if nz.any() else 0.0


def forward_bounds(y, gamma, beta, st, mm=None, mv=None, momentum=MOMENTUM):
    sc = gamma * st.rstd
    b = SimpleNamespace(mean=U * np.abs(st.mean), rstd=4 * U * st.rstd, scale=5 * U * np.abs(sc),
                        shift=U * (8 * np.abs(st.mean * sc) + np.abs(beta)),
                        out=8 * U * (np.abs(y * sc) + np.abs(st.mean * sc) + np.abs(beta)))
    if mm is not None:
        m = float(np.float32(momentum))
        b.moving_mean = U * (2 * np.abs(mm * m) + 3 * np.abs(st.mean * (1 - m)))
        b.moving_var = U * (2 * np.abs(mv * m) + 3 * np.abs(st.unbiased * (1 - m)))
    return b


def backward_bounds(dout, y, scale, shift, mean, rstd, gamma, count, L, relu=True):
    r = backward(dout, y, scale, shift, mean, rstd, gamma, count, relu)
    amb = (np.abs(r.v) <= 4 * U * (np.abs(y * scale) + np.abs(shift))) if relu else np.zeros(r.v.shape, bool)
    e = 3 * (np.abs(y) + np.abs(mean)) * rstd
    adz, axh = np.abs(r.dz), np.abs(r.xhat)
    amb1, amb2 = (np.abs(dout) * amb).sum(0), (np.abs(dout) * axh * amb).sum(0)
    s1 = U * L * adz.sum(0) + amb1
    s2 = U * (L * (adz * axh).sum(0) + (adz * e).sum(0)) + amb2
    k0, k1, k2 = np.abs(r.coef)
    dy = k0 * (U * (4 * (adz + k1 + axh * k2) + e * k2) + (s1 + axh * s2) / count)
    return SimpleNamespace(ref=r, amb=amb, s1=s1, s2=s2, dy=dy, left_out=int(amb.sum()))


# ----------------------------------------------------------------------------------------------
# exact data (section 1 of tests/test_bn_gpu.py): integers and dyadic constants, every result independent of order and contraction
# ----------------------------------------------------------------------------------------------
APPLY_SHAPES = [(8, 1), (8, 1000), (64, 1), (64, 1000), (2048, 64)]                  # c, npix
REDUCE_SHAPES = [(8, 1), (8, 1000), (64, 1000), (256, 32776), (2048, 64)]
Y_AMP = {torch.bfloat16: 100, torch.float16: 1000, torch.float32: 1000}                # forward: the 16-bit store must round
_cache = {}


def clear_cache():
    _cache.clear()


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _ints(g, shape, lo, hi, density=1.0):
    v = g.randint(lo, hi + 1, size=shape).astype(F64)
    if density < 1.0:
        v = np.where(g.random_sample(shape) < density, v, 0.0)               # (not v * mask: that leaves -0.0)
    return v


def exact_channels(c, seed):
    """mean integer, rstd a power of two, gamma = k/8 (channel 1 negative, channel 2 zero), beta = j/4 (0 in half the channels,
    and with mean 0 in every fourth: there y == 0 sits on the ReLU edge); coef: k0 = gamma rstd, k1 = j/32, k2 = j/64."""
    g = np.random.RandomState(seed)
    ch = np.arange(c)
    mean = _ints(g, c, -2, 2)
    rstd = 2.0 ** _ints(g, c, -2, 1)
    k = _ints(g, c, 1, 16) * np.where(g.random_sample(c) < 0.3, -1.0, 1.0)
    k[1], k[2] = -abs(k[1]), 0.0
    gamma = k / 8
    beta = np.where(ch % 2 == 0, 0.0, _ints(g, c, -8, 8) / 4)
    mean[ch % 4 == 0] = 0.0
    scale = gamma * rstd
    coef = np.stack([scale, _ints(g, c, -31, 31) / 32, _ints(g, c, -31, 31) / 64])
    return SimpleNamespace(mean=mean, rstd=rstd, gamma=gamma, beta=beta, scale=scale, shift=beta - mean * scale, coef=coef)


def exact_case(c, npix, amp=4):
    """y (integers in [-amp, amp], half of them 0), dout (integers in [-3, 3], 60 % non-zero) and the channel constants."""
    def build():
        e = exact_channels(c, 7 * c + npix)
        g = np.random.RandomState(c + 3 * npix + amp)
        e.y = _ints(g, (npix, c), -amp, amp, 0.5)
        e.dout = _ints(g, (npix, c), -3, 3, 0.6)
        e.c, e.npix = c, npix
        return e
    return cached(('exact', c, npix, amp), build)


def exact_up(B, h, w, c):
    """Multiples of 4 for the up-sampling kernels (weights 1/4, 1/2, 1: every adjoint an integer), a mask input dense in zeros."""
    def build():
        e = exact_channels(c, 11 * c + h)
        g = np.random.RandomState(B * 100 + h + w + c)
        e.dy_up = 4 * _ints(g, (B, 2 * h, 2 * w, c), -2, 2)
        e.x = 4 * _ints(g, (B, h, w, c), -6, 6, 0.7)
        e.mask = _ints(g, (B, h, w, c), -3, 5, 0.7)
        e.y = _ints(g, (B, h, w, c), -4, 4, 0.5)
        return e
    return cached(('up', B, h, w, c), build)


def up_fwd(x):
    """out[2i] = in[i], out[2i+1] = (in[i] + in[min(i+1, n-1)])/2 along both axes."""
    def axis(a, ax):
        nxt = np.concatenate([np.take(a, range(1, a.shape[ax]), ax), np.take(a, [a.shape[ax] - 1], ax)], ax)
        o = np.stack([a, (a + nxt) / 2], ax + 1)
        return o.reshape(a.shape[:ax] + (2 * a.shape[ax],) + a.shape[ax + 1:])
    return axis(axis(x, 2), 1)


def up_bwd(dy):
    """The adjoint of up_fwd."""
    def axis(d, ax):
        n = d.shape[ax] // 2
        even, odd = np.take(d, range(0, 2 * n, 2), ax), np.take(d, range(1, 2 * n, 2), ax)
        o = even + odd / 2                                                   # in[i] from out[2i] and out[2i+1]
        sl = [slice(None)] * d.ndim
        sl[ax] = slice(1, n)
        o[tuple(sl)] += np.take(odd, range(0, n - 1), ax) / 2               # in[i] from out[2i-1]
        sl[ax] = slice(n - 1, n)
        o[tuple(sl)] += np.take(odd, [n - 1], ax) / 2                        # the clamped neighbour of the last sample is itself
        return o
    return axis(axis(dy, 1), 2)


FINALIZE_ROWS = {32: [1, 63, 64, 65, 256, 257, 449, 512, 513, 1023, 1024, 1025, 1793, 2048, 2049, 4096], 8: [1, 1024, 2049],
                 12: [1100], 10: [40]}
FINALIZE_CASES = [(c, n) for c, ns in FINALIZE_ROWS.items() for n in ns]


def finalize_ldp(c):
    return c if c == 10 else c + 8                                           # c = 10: the scalar path needs ldp == c


def table(nblk, c, ldp, seed=0):
    """Integer partial rows [nblk][2][ldp] (f32): first sums in [-20, 20], second sums in [400, 2000] (a variance that is not
    clamped); columns [c, ldp) NaN.  Independent random rows: a row taken twice in place of its neighbour changes every total."""
    def build():
        g = np.random.RandomState(nblk * 131 + c + seed)
        t = np.full((nblk, 2, ldp), np.nan, np.float32)
        t[:, 0, :c] = _ints(g, (nblk, c), -20, 20)
        t[:, 1, :c] = _ints(g, (nblk, c), 400, 2000)
        return t
    return cached(('table', nblk, c, ldp, seed), build)


FUSED_ROWS = [1, 15, 16, 17, 32, 33, 127, 128, 129, 144, 145, 255, 256]
FUSED_CASES = [(c, 1024, n) for c in (32, 256) for n in FUSED_ROWS] + [(c, n, r) for c in (32, 256) for n in (256, 4096) for r in (17, 145)]


def fused_table(nblk, c):
    """Integer rows in [-4, 4] for imm_bn_bwd_apply_fused: at a power-of-two count k1 = S1/N and k2 = S2/N are dyadic."""
    g = np.random.RandomState(nblk * 17 + c)
    return _ints(g, (nblk, 2, c), -4, 4).astype(np.float32)


ROWS_REDUCE = [(700, 64, 32), (33, 520, 32), (257, 16, 7), (64, 64, 1), (1, 64, 32)]
UP_SHAPES = [(3, 8, 24, 16), (2, 8, 8, 64)]
COLSUM_SHAPES = [(8, 1), (8, 1000), (2048, 1), (2048, 1000)]


def exact_in_f32(v):
    v = np.asarray(v, F64)
    return bool((v.astype(np.float32).astype(F64) == v).all())


def stored_bits(v64, dt):
    """What a kernel stores for the f32 value nearest v64: that value (f32 storage) or its one RNE to dt (exact_data.rne16)."""
    t = torch.from_numpy(np.ascontiguousarray(v64, dtype=F64)).float()
    return t if dt == torch.float32 else rne16(t.double(), dt)


# ----------------------------------------------------------------------------------------------
# bounded data (section 2): real values, ill-conditioned and degenerate channels
# ----------------------------------------------------------------------------------------------
BOUNDED_SHAPES = [(32, 1000, 7), (64, 65, 1), (256, 512, 33), (32, 1, 1), (128, 4096, 145)]          # c, npix, partial rows
CH_NEG, CH_ZERO, CH_R8, CH_R64, CH_CONST, CH_DEAD = 1, 2, 3, 4, 5, 6


def bounded_case(c, npix, nrows, dt):
    """y = 2 randn + offset: mean/deviation 0.25, one channel 8, one 64, one constant 0.5; gamma = 1 + randn/2 with one negative and
    one zero channel; beta = randn/2, one channel -100 (dead behind the ReLU).  rows: the f32 sums of `nrows` pixel ranges."""
    def build():
        g = np.random.RandomState(c * 13 + npix)
        off = np.full(c, 0.5)
        off[CH_R8], off[CH_R64] = 16.0, 128.0
        y = 2.0 * g.standard_normal((npix, c)) + off
        y[:, CH_CONST] = 0.5
        gamma = f32(1.0 + 0.5 * g.standard_normal(c)).astype(F64)
        gamma[CH_NEG], gamma[CH_ZERO] = -abs(gamma[CH_NEG]) - 0.25, 0.0
        beta = f32(0.5 * g.standard_normal(c)).astype(F64)
        beta[CH_DEAD] = -100.0
        e = SimpleNamespace(c=c, npix=npix, nrows=nrows, dt=dt, gamma=gamma, beta=beta)
        e.y_t = store(y, dt)
        e.y = widen(e.y_t)
        e.dout_t = store(g.standard_normal((npix, c)), dt)
        e.dout = widen(e.dout_t)
        e.mm = f32(0.3 * g.standard_normal(c)).astype(F64)
        e.mv = f32(1.0 + np.abs(0.2 * g.standard_normal(c))).astype(F64)
        idx = np.linspace(0, npix, nrows + 1).astype(int)
        e.rows = np.stack([np.stack([e.y[a:b].sum(0), (e.y[a:b] ** 2).sum(0)]) for a, b in zip(idx[:-1], idx[1:])]).astype(np.float32)
        e.st = stats(e.rows, npix)
        e.fwd = forward(e.y, gamma, beta, e.st)
        # what the backward kernels are handed: the f32 per-channel arrays
        e.scale, e.shift = f32(e.fwd.scale).astype(F64), f32(e.fwd.shift).astype(F64)
        e.mean, e.rstd = f32(e.st.mean).astype(F64), f32(e.st.rstd).astype(F64)
        e.geo = bwd_geometry(npix, c)
        return e
    return cached(('bounded', c, npix, nrows, dt), build)


def left_out_cap(npix, c):
    return math.floor(1e-3 * npix * c)
