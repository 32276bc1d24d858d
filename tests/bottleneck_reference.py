"""The landmark bottleneck and the pose head as imm_amd/csrc/bottleneck.hip states them, in numpy f64, with a-priori rounding bounds
and the data of tests/test_bottleneck_cpu.py and tests/test_bottleneck_gpu.py.  No autograd, no GPU; torch only rounds to bf16 / f16
(through bn_reference).

The rule (heat [B, h, w, K]; lin_n(i) = -1 + 2 i / (n - 1), -1 for n == 1; s = side of the maps; i2 = inv_std^2)
    means      r[y] = sum_x heat[y, x] / w        c[x] = sum_y heat[y, x] / h
    softmax    py = exp(r - max r) / sum, px alike;   mu = (sum_y py[y] lin_h(y), sum_x px[x] lin_w(x))
    offsets    dy = lin_s(yy) - mu_y,  dx = lin_s(xx) - mu_x         (f32 subtractions of the kernel's own f32 mu: emulated exactly)
    rot        G = exp(-(dy^2 + dx^2) i2)                             dG/dmu = G 2 i2 (dy, dx)
    flat       d = (dy^2 + dx^2) i2 + 1e-5f,  G = exp(-d^(1/4))       dG/dmu = G d^(-3/4) / 4 * 2 i2 (dy, dx)
    ankush     r_a = sqrt(1e-4f + |d_a| inv_std),  G = exp(-r_y) exp(-r_x)     dG/dmu_a = G inv_std sign(d_a) / (2 r_a),  sign(0) = 0
    backward   dmu = sum_p dG[p] dG/dmu[p];   drow[y] = py[y] (lin_h(y) - mu_y) dmu_y,  dcol alike;   dheat[y, x] = drow[y] / w + dcol[x] / h
    pose head  heat = feat W + bias (forward);   dfeat[p][c] = sum_k dheat16[p][k] W[c][k],  bias partial[k] = sum_p dheat16[p][k], both
               from the STORED 16-bit dheat

What is reproduced in f32, operation for operation, because it is reproducible: lin_pm1 (one exact product, one correctly rounded
division, one addition; it differs from the oracle's linspace in the last place for some n, e.g. n = 12: the kernel's expression is
the definition), the row and column means of integer data, and every `lin - mu`.  Everything downstream of those is f64.

Bounds.  u = 2^-24 (half an ulp of f32, relative); first order, every bound times 1 + 2^-10; one rounding per f32 operation, a
contracted multiply-add has fewer, never more.  The device functions' accuracy cannot be derived here and no HIP math documentation
is installed next to the compiler, so these are ASSUMPTIONS, not measurements: division and sqrtf good to 1 ulp, expf to 2, powf to
4 (ULP_*; 1 ulp <= 2 u relative).  A result below the smallest normal f32 may be flushed: every bound carries 2^-126 absolute.

    mean       w additions act on at most sum |x| (w u mean|x|), the quotient 2 u |mean|
    softmax    z = r - max: u |z| and the error of r (the error of max shifts numerator and denominator alike and cancels);
               e = expf(z): relative e_z (the slope of exp) + 4 u;  den: n additions (n u) on terms that carry their own error
               (weighted by p);  p = e / den: 2 u.   rel p = e_z + 4 u + sum_j p_j (e_z_j + 4 u) + n u + 2 u
    mu         n multiply-adds: sum |lin| e_p + n u sum |p lin|     (lin itself is the kernel's f32 value: no error)
    maps       the argument's error times the slope, plus the function:
               rot     a = (dy^2 + dx^2) i2: 4 roundings, all on positive terms: 4 u a;   G (4 u a + 4 u)
               flat    d: 5 u;  t = powf(d, 1/4): 5/4 u + 8 u;   G (t 9.25 u + 4 u)
               ankush  r = sqrtf(1e-4f + |d| inv_std): product, sum (2 u, halved by the root) + 2 u = 3 u;  a factor exp(-r): 3 u r + 4 u;
                       G ((r_y + r_x) 3 u + 8 u + u)
    dG/dmu     relative, on each term t = dG * dG/dmu  (REL_*):
               rot     G (4 a + 4) and the products with i2, d_a and dG: + 3
               flat    G (9.25 t + 4), powf(d, -3/4): 3.75 + 8, four products: + 4
               ankush  G ((r_y + r_x) 3 + 8 + 1), r_a in the divisor 3, inv_std 1, the quotient 2, dG 1
    dmu        depth(s, NTHR) = trips of a thread (ceil(s s / NTHR)) + six butterfly steps + NTHR / 64 rows, on sum |t|, plus sum |t| rel(t).
               NTHR is 256 standalone and 512 in the pose head, yet the fused dheat equals the standalone one bit for bit only while
               the order agrees, which the GPU test asserts where it does (one trip, s s <= 256).  A single non-zero dG per landmark makes
               the sum one product: depth 1
    drow       |py (lin - mu)| e_dmu + 2 u |drow|   (two products; lin - mu is emulated)
    dheat      e_drow / w + e_dcol / h + 2 u (|drow| / w + |dcol| / h) (the two quotients) + u |dheat| (the sum)
    dfeat      K products of 16-bit values are exact; the matrix instruction's additions are not documented as correctly rounded:
               1 ulp each, 2 K u sum |dheat16 W|; then the one 16-bit store
    bias       h w u sum |dheat16| (h w additions at most, in any order)
    16-bit     the window rule: the stored value lies in [RNE(ref - bound), RNE(ref + bound)] (window); f32 storage |got - ref| <= bound

Nothing is left out of any comparison: the backward is a function of the f32 inputs the kernel is handed, the sign decisions of
'ankush' are taken on the emulated f32 offsets, and at the kink (a pixel on a landmark) every mode's gradient term is exactly 0.
"""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bn_reference import F64, STORAGE, STORAGE_IDS, U, exact_in_f32, half_ulp, ratio, store, stored_bits, violations, widen  # noqa: E402,F401

SLACK = 1.0 + 2.0 ** -10
TINY = 2.0 ** -126
ULP_DIV, ULP_SQRT, ULP_EXP, ULP_POW = 1, 1, 2, 4            # assumed accuracy of the device functions, in ulps (1 ulp <= 2 u)
MODES = ['rot', 'flat', 'ankush']
C5, C4 = float(np.float32(1e-5)), float(np.float32(1e-4))
BF16, F16, F32T = STORAGE
BT_THREADS, PH_BWD_THREADS, KC = 256, 512, 10
P_EXACT, SHIFT = 256, 8192
INV_STDS = (10.0, 3.0)           # every shipped configuration's, and a wide one: both squares are exact in f32
_cache = {}


def clear_cache():
    _cache.clear()


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


# ----------------------------------------------------------------------------------------------
# f32 emulation of the reproducible parts
# ----------------------------------------------------------------------------------------------
def lin_pm1(n):
    """The kernel's lin_pm1(i, n) for i in range(n), as f32."""
    if n == 1:
        return np.array([-1.0], np.float32)
    i = np.arange(n, dtype=np.float32)
    return np.float32(-1.0) + (np.float32(2.0) * i) / np.float32(n - 1)


def means_f32(heat):
    """Row and column means as the kernel takes them: a sequential f32 sum, then one division.  heat [B, h, w, K]."""
    x = np.asarray(heat).astype(np.float32)
    _B, h, w, _K = x.shape
    racc, cacc = np.zeros_like(x[:, :, 0]), np.zeros_like(x[:, 0])
    for j in range(w):
        racc = racc + x[:, :, j]
    for j in range(h):
        cacc = cacc + x[:, j]
    return racc / np.float32(w), cacc / np.float32(h)


def softargmax_f32(heat):
    """The f32 soft-argmax of an EXACT heat-map: the winners' exponent is expf(0) = 1, every other argument lies below -104, where
    expf is 0 in f32 whatever its accuracy.  Anything in between makes the result NaN (the premise failed).  Returns mu [B, K, 2],
    py, px and the largest loser's argument."""
    rm, cm = means_f32(heat)
    out, worst = [], -np.inf
    for v in (rm, cm):
        n = v.shape[1]
        z = v - v.max(1, keepdims=True)
        losers = z[z != 0]
        worst = max(worst, float(losers.max()) if losers.size else -np.inf)
        e = np.where(z == 0, np.float32(1), np.where(z < -104, np.float32(0), np.float32(np.nan)))
        den = np.zeros_like(e[:, 0])
        for j in range(n):
            den = den + e[:, j]
        lin, ex, p = lin_pm1(n), np.zeros_like(den), e / den[:, None]
        for j in range(n):
            prod = p[:, j].astype(F64) * float(lin[j])
            assert exact_in_f32(prod), 'p * lin must be exact for the multiply-add to round once'
            ex = (ex.astype(F64) + prod).astype(np.float32)
        out.append((ex, p))
    return np.stack([out[0][0], out[1][0]], -1), out[0][1], out[1][1], worst


def offsets(mu32, s):
    """dy [B, s, K], dx [B, s, K]: the f32 differences lin_s - mu (f32 - f32 rounds once, as the kernel's does), widened."""
    mu32 = np.asarray(mu32)
    lin = lin_pm1(s)[None, :, None]
    return (lin - mu32[:, None, :, 0]).astype(F64), (lin - mu32[:, None, :, 1]).astype(F64)


# ----------------------------------------------------------------------------------------------
# the rule in f64
# ----------------------------------------------------------------------------------------------
def forward(heat):
    """heat [B, h, w, K] f64 -> rmean, cmean, py, px, mu [B, K, 2]."""
    heat = np.asarray(heat, F64)
    _B, h, w, _K = heat.shape
    r = SimpleNamespace(rmean=heat.sum(2) / w, cmean=heat.sum(1) / h)
    mus = []
    for name, v, n in (('py', r.rmean, h), ('px', r.cmean, w)):
        z = v - v.max(1, keepdims=True)
        e = np.exp(z)
        p = e / e.sum(1, keepdims=True)
        setattr(r, name, p)
        mus.append((p * lin_pm1(n).astype(F64)[None, :, None]).sum(1))
    r.mu = np.stack(mus, -1)
    return r


def gauss_value(dy, dx, inv_std, mode):
    i2 = inv_std * inv_std
    if mode == 'rot':
        return np.exp(-(dy * dy + dx * dx) * i2)
    if mode == 'flat':
        return np.exp(-((dy * dy + dx * dx) * i2 + C5) ** 0.25)
    return np.exp(-np.sqrt(C4 + np.abs(dy) * inv_std)) * np.exp(-np.sqrt(C4 + np.abs(dx) * inv_std))


def gauss_grad(dy, dx, inv_std, mode):
    """G and dG/dmu_y, dG/dmu_x at the offsets (coord - mu)."""
    i2 = inv_std * inv_std
    g = gauss_value(dy, dx, inv_std, mode)
    if mode == 'rot':
        return g, g * 2 * i2 * dy, g * 2 * i2 * dx
    if mode == 'flat':
        d = (dy * dy + dx * dx) * i2 + C5
        c = g * 0.25 * d ** -0.75 * 2 * i2
        return g, c * dy, c * dx
    ry, rx = np.sqrt(C4 + np.abs(dy) * inv_std), np.sqrt(C4 + np.abs(dx) * inv_std)
    return g, g * inv_std * np.sign(dy) / (2 * ry), g * inv_std * np.sign(dx) / (2 * rx)


def _grid(mu32, s):
    dy, dx = offsets(mu32, s)
    return dy[:, :, None, :], dx[:, None, :, :]                    # [B, s, 1, K], [B, 1, s, K]


def render(mu32, s, inv_std, mode):
    """The maps [B, s, s, K] of the f32 landmarks mu32 and their bound (before the store)."""
    dy, dx = _grid(mu32, s)
    g = gauss_value(dy, dx, inv_std, mode)
    i2 = inv_std * inv_std
    a = (dy * dy + dx * dx) * i2
    if mode == 'rot':
        rel = 4 * a + 2 * ULP_EXP
    elif mode == 'flat':
        rel = (a + C5) ** 0.25 * (1.25 + 2 * ULP_POW) + 2 * ULP_EXP
    else:
        ry, rx = np.sqrt(C4 + np.abs(dy) * inv_std), np.sqrt(C4 + np.abs(dx) * inv_std)
        rel = (ry + rx) * (1 + 2 * ULP_SQRT) + 4 * ULP_EXP + 1
    return g, g * rel * U * SLACK + TINY


def on_landmark(inv_std, mode):
    """The one value a mode defines at the pixel that sits on the landmark (dy = dx = 0), and its bound."""
    z = np.zeros((1, 1, 1))
    mu = np.full((1, 1, 2), -1.0, np.float32)
    g, b = render(mu, 1, inv_std, mode)                            # s = 1: the only pixel is lin = -1 = mu
    assert float(gauss_value(z, z, inv_std, mode)[0, 0, 0]) == float(g[0, 0, 0, 0])
    return float(g[0, 0, 0, 0]), float(b[0, 0, 0, 0])


def grad_rel(dy, dx, inv_std, mode):
    """Relative error of one term dG * dG/dmu_a, in units of u (the same for both axes but for 'ankush', where the larger is taken)."""
    i2 = inv_std * inv_std
    a = (dy * dy + dx * dx) * i2
    if mode == 'rot':
        return 4 * a + 2 * ULP_EXP + 3
    if mode == 'flat':
        t = (a + C5) ** 0.25
        return t * (1.25 + 2 * ULP_POW) + 2 * ULP_EXP + (3.75 + 2 * ULP_POW) + 4
    ry, rx = np.sqrt(C4 + np.abs(dy) * inv_std), np.sqrt(C4 + np.abs(dx) * inv_std)
    return (ry + rx) * (1 + 2 * ULP_SQRT) + 4 * ULP_EXP + 1 + (1 + 2 * ULP_SQRT) + 1 + 2 * ULP_DIV + 1


def depth(s, nthr):
    """Additions on the longest chain of the dmu reduction: trips of a thread, six butterfly steps, NTHR / 64 rows."""
    return -(-s * s // nthr) + 6 + nthr // 64


def backward(dg, mu32, py32, px32, inv_std, mode, nthr=BT_THREADS, single=False):
    """dheat [B, h, w, K] and its bound from what the kernel is handed: dg [B, s, s, K] (the stored values, widened), the f32 mu, py, px."""
    dg = np.asarray(dg, F64)
    mu32, py, px = np.asarray(mu32), np.asarray(py32, F64), np.asarray(px32, F64)
    s, h, w = dg.shape[1], py.shape[1], px.shape[1]
    dy, dx = _grid(mu32, s)
    _g, gmy, gmx = gauss_grad(dy, dx, inv_std, mode)
    rel = grad_rel(dy, dx, inv_std, mode)
    D = 1 if single else depth(s, nthr)
    r = SimpleNamespace(depth=D)
    dmu, e_dmu = [], []
    for gm in (gmy, gmx):
        t = dg * gm
        dmu.append(t.sum((1, 2)))
        e_dmu.append(U * ((np.abs(t) * rel).sum((1, 2)) + D * np.abs(t).sum((1, 2))))
    r.dmu, r.e_dmu = np.stack(dmu, -1), np.stack(e_dmu, -1)                       # [B, K, 2]
    parts = []
    for a, p, n in ((0, py, h), (1, px, w)):
        l = (lin_pm1(n)[None, :, None] - mu32[:, None, :, a]).astype(F64)         # [B, n, K]
        d = p * l * r.dmu[:, None, :, a]
        parts.append((d, np.abs(p * l) * r.e_dmu[:, None, :, a] + 2 * U * np.abs(d)))
    (r.drow, e_row), (r.dcol, e_col) = parts
    qr, qc = r.drow[:, :, None, :] / w, r.dcol[:, None, :, :] / h
    r.dheat = qr + qc
    r.bound = (e_row[:, :, None, :] / w + e_col[:, None, :, :] / h + 2 * ULP_DIV * U * (np.abs(qr) + np.abs(qc))
               + U * np.abs(r.dheat)) * SLACK + TINY
    return r


def forward_bounds(heat):
    """forward(heat) with e_py, e_px, e_mu [B, K, 2]."""
    heat = np.asarray(heat, F64)
    _B, h, w, _K = heat.shape
    r = forward(heat)
    A = np.abs(heat)
    e_mu = []
    for name, v, ev, n in (('py', r.rmean, U * (w * A.sum(2) / w + 2 * ULP_DIV * np.abs(r.rmean)), h),
                           ('px', r.cmean, U * (h * A.sum(1) / h + 2 * ULP_DIV * np.abs(r.cmean)), w)):
        p = getattr(r, name)
        z = v - v.max(1, keepdims=True)
        rel_e = ev + U * np.abs(z) + 2 * ULP_EXP * U
        rel_p = rel_e + (p * rel_e).sum(1, keepdims=True) + n * U + 2 * ULP_DIV * U
        e_p = p * rel_p * SLACK + TINY
        setattr(r, 'e_' + name, e_p)
        lin = np.abs(lin_pm1(n).astype(F64))[None, :, None]
        e_mu.append(((lin * e_p).sum(1) + n * U * (p * lin).sum(1)) * SLACK)
    r.e_mu = np.stack(e_mu, -1)
    return r


def head_dgrad(dheat16, wtd, K):
    """dfeat [.., C] = dheat16 [.., :K] wtd[:, :K]^T in f64 and its bound before the 16-bit store; the bias partial [B, K] and its bound."""
    d, wd = np.asarray(dheat16, F64)[..., :K], np.asarray(wtd, F64)[:, :K]
    ref = d @ wd.T
    bound = 2 * K * U * (np.abs(d) @ np.abs(wd).T) * SLACK + TINY
    npix = d.shape[1] * d.shape[2]
    return ref, bound, d.sum((1, 2)), npix * U * np.abs(d).sum((1, 2)) * SLACK + TINY


def window(got, ref, bound, dt):
    """Elements of `got` (widened) outside [RNE_dt(ref - bound), RNE_dt(ref + bound)]; for f32 storage outside ref +- bound.  A NaN is outside."""
    got, ref, bound = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(bound, F64)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    assert np.isfinite(ref).all() and np.isfinite(bound).all() and (bound >= 0).all(), 'the REFERENCE or its bound: a bug of the test'
    if dt == torch.float32:
        return ~(np.abs(got - ref) <= bound)
    lo, hi = widen(store(ref - bound, dt)), widen(store(ref + bound, dt))
    return ~((got >= lo) & (got <= hi))


# ----------------------------------------------------------------------------------------------
# data
# ----------------------------------------------------------------------------------------------
def index_sets(n):
    """The winning rows (columns) a landmark may have on an axis of n: the first, the last, the symmetric pair (mu == 0 exactly), an
    asymmetric pair (mu off the grid), one in the middle, four."""
    sets = [[0], [n - 1]]
    if n >= 2:
        sets.append([0, n - 1])
    if n >= 3:
        sets += [[0, 1], [n // 2]]
    if n >= 5:
        sets += [[1, n - 1], [0, 1, n - 2, n - 1], [0, 1, 2, 4]]
    return sets


def predicted(idx, n):
    """p and mu of the softmax whose winners are idx: p = 1 / |idx| there, mu the f32 sum of the exact products in ascending order."""
    p = np.zeros(n, np.float32)
    p[idx] = np.float32(1.0) / np.float32(len(idx))
    lin, mu = lin_pm1(n), np.float32(0)
    for j in sorted(idx):
        mu = np.float32(mu + p[j] * lin[j])
    return p, mu


def exact_heat(h, w, K, B=2):
    """heat[b, y, x, k] = 256 ([y in Y_bk] + [x in X_bk]), the predicted py, px, mu, and the sets."""
    def build():
        sy, sx = index_sets(h), index_sets(w)
        e = SimpleNamespace(h=h, w=w, K=K, B=B, heat=np.zeros((B, h, w, K)), py=np.zeros((B, h, K), np.float32),
                            px=np.zeros((B, w, K), np.float32), mu=np.zeros((B, K, 2), np.float32), sets=[])
        for b in range(B):
            for k in range(K):
                Y, X = sy[(k + 3 * b) % len(sy)], sx[(k // len(sy) + 2 * k + b) % len(sx)]
                e.sets.append((b, k, Y, X))
                e.heat[b, Y, :, k] += P_EXACT
                e.heat[b, :, X, k] += P_EXACT
                e.py[b, :, k], e.mu[b, k, 0] = predicted(Y, h)
                e.px[b, :, k], e.mu[b, k, 1] = predicted(X, w)
        return e
    return cached(('exact', h, w, K, B), build)


def one_hot_heat(h, w, K, B=2):
    """A saturated softmax: one winning row and one winning column per landmark, spread over the whole map (edges included)."""
    def build():
        e = SimpleNamespace(h=h, w=w, K=K, B=B, heat=np.zeros((B, h, w, K)), py=np.zeros((B, h, K), np.float32),
                            px=np.zeros((B, w, K), np.float32), mu=np.zeros((B, K, 2), np.float32))
        for b in range(B):
            for k in range(K):
                y, x = (k * 3 + b) % h, (k * 5 + 2 * b + (h - 1 if k == 1 else 0)) % w
                if k == 0:
                    y, x = 0, w - 1
                e.heat[b, y, :, k] += P_EXACT
                e.heat[b, :, x, k] += P_EXACT
                e.py[b, y, k] = e.px[b, x, k] = 1
                e.mu[b, k] = lin_pm1(h)[y], lin_pm1(w)[x]
        return e
    return cached(('onehot', h, w, K, B), build)


def bump_heat(B, h, w, K, seed=0):
    """A negative quadratic bump per landmark (centres uniform in [-1, 1]^2, sharpness 40) plus randn / 2, as the f32 the kernel reads."""
    def build():
        g = np.random.RandomState(1000 + seed + 7 * h + 13 * w + K)
        c = g.uniform(-1, 1, (B, K, 2))
        ly, lx = lin_pm1(h).astype(F64)[None, :, None, None], lin_pm1(w).astype(F64)[None, None, :, None]
        v = -40.0 * ((ly - c[:, None, None, :, 0]) ** 2 + (lx - c[:, None, None, :, 1]) ** 2) + 0.5 * g.standard_normal((B, h, w, K))
        return v.astype(np.float32)
    return cached(('bump', B, h, w, K, seed), build)


def randn_heat(B, h, w, K, T, seed=0):
    def build():
        g = np.random.RandomState(2000 + seed + 7 * h + 13 * w + K + int(T))
        return (T * g.standard_normal((B, h, w, K))).astype(np.float32)
    return cached(('randn', B, h, w, K, T, seed), build)


def real_heat(family, B, h, w, K):
    return bump_heat(B, h, w, K) if family == 'bump' else randn_heat(B, h, w, K, {'flat2': 2.0, 'sat30': 30.0}[family])


FAMILIES = ['bump', 'flat2', 'sat30']


def dense_dg(B, s, K, dt, seed=0):
    """randn rounded to dt: values that round in the storage type.  Returns the tensor of type dt."""
    def build():
        g = np.random.RandomState(3000 + seed + s + 5 * K)
        return store(g.standard_normal((B, s, s, K)), dt)
    return cached(('dense', B, s, K, dt, seed), build)


def single_dg(B, s, K, dt, seed=0):
    """One non-zero value per (sample, landmark), at a random pixel."""
    def build():
        g = np.random.RandomState(4000 + seed + s + 5 * K)
        v = np.zeros((B, s * s, K))
        for b in range(B):
            for k in range(K):
                v[b, g.randint(s * s), k] = g.standard_normal() + (2.0 if g.rand() < 0.5 else -2.0)
        return store(v.reshape(B, s, s, K), dt)
    return cached(('single', B, s, K, dt, seed), build)


def ints(shape, lo, hi, seed):
    return np.random.RandomState(seed).randint(lo, hi + 1, size=shape).astype(F64)


def selector(C, K, lddh, seed=0):
    """The data-gradient filter wtd [C][lddh] with W[c][k] = +-2^e (e in 0..2) at k = c % K, else 0 (zero in the columns [K, lddh))."""
    g = np.random.RandomState(5000 + seed + C + K)
    w = np.zeros((C, lddh))
    w[np.arange(C), np.arange(C) % K] = 2.0 ** g.randint(0, 3, C) * np.where(g.rand(C) < 0.5, -1.0, 1.0)
    return w


def rounds_in(v64, dt):
    """Share of the values that are not representable in dt."""
    v64 = np.asarray(v64, F64)
    return float((widen(store(v64, dt)) != v64).mean()) if dt != torch.float32 else float((v64.astype(np.float32).astype(F64) != v64).mean())


def fwd_lds(h, w, K):
    return 4 * (h * w * K + (h + w) * K + 2 * K)


def bwd_lds(h, w, K, lddh):
    return 4 * (((2 + h + w) * K + 3) // 4 * 4 + PH_BWD_THREADS) + h * w * lddh * 2


LDS_CAP, LDS_OPT_IN = 160 * 1024 - 1024, 64 * 1024
