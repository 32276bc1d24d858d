"""The tail of the step as imm_amd/csrc/loss_optim.hip states it, in numpy f64: the masked error sums, imm_perceptual_finalize, the
gradient injection at the taps and imm_clip_adam_step, with a-priori rounding bounds and the data of tests/test_loss_cpu.py and
tests/test_loss_gpu.py.  No autograd, no GPU; torch only rounds to bf16 / f16 (through bn_reference).

The rule
    sse           sum_p mask[b, y r, x r] sum_ch f(a - b),  r = S / s,  f = square (l2) or abs (l1)
    finalize      m = SSE / nel;  wl = agg + 0.01f (m - agg);  term = m / wl;  coef = ls 1000 (1/wl - 0.01f m / wl^2) k / nel with
                  k = 2 (l2) or 1 (l1);  rec = 1000 sum term;  out = {term[n], m[n], coef[n], rec, wd, rec + wd};  agg <- wl when
                  training.  Mode L2: out = {m, m, ls (1000/255) 2 / nel, 1000 m, wd, 1000 m / 255 + wd}
    tap_grad      v = d_in + coef mask e,  e = ap - ag or its sign (l1);  v = 0 where relu and not ap > 0
    unpool_tap    v = [p is the FIRST maximum of its 2x2 window, order (0,0) (0,1) (1,0) (1,1)] dpool + coef mask (ap - ag); 0 unless ap > 0
    image_grad    dpred[p][ch < 3] = (coef mask[p]) e,  dpred[p][ch >= 3] = +0
    prepare       g' = g (grad_scale / S) + wd w;  chunk sums of g'^2;  norm2 = (float) of their f64 sum per tensor
    clip          factor = clip / max(sqrtf(norm2), clip)  (1 when clip == 0);  gc = g' factor
    adam          m = b1 m + (1 - b1) gc;  v = b2 v + (1 - b2) gc gc;  w -= lr_t m / (sqrt(v) + eps)
    adadelta      v = rho v + (1 - rho) gc gc;  u = sqrt(m + eps) / sqrt(v + eps) gc;  m = rho m + (1 - rho) u u;  w -= lr u
    adagrad       v += gc gc;  w -= lr gc / sqrt(v)
    learning rate lr = lr_multiple lr_start lr_decay^(global_step // lr_step);  lr_t = lr sqrt(1 - b2^t) / (1 - b1^t),  t = adam_t + 1

Bounds.  u = 2^-24 (half an ulp of f32, relative).  One rounding per f32 operation; a contracted multiply-add has fewer, never
more.  Division and sqrtf are taken as good to 1 ulp = 2 u.  f64 steps of the kernels (the sums over partials, SSE / nel, the
learning rate before its cast) count 0.  e_x is the absolute bound of x; every bound is multiplied by 1 + 2^-10 for the
second-order terms the first-order count drops.

    finalize   m      1 on |m|: the cast
               wl     e_m 0.01 (m carries it through the product);  1 on |m - agg| 0.01 (the subtraction) + 1 on the product
                      0.01 |m - agg| + 1 on |wl| (the sum)  =  u (0.01 |m| + 0.02 |m - agg| + |wl|)
               term   e_m / wl + |m| e_wl / wl^2 + 2 u |term|
               coef   A = 1/wl: e_A = e_wl / wl^2 + 2 u A.   B = 0.01f m / (wl wl): relative 1 (m) + 1 (0.01f m) + 1 (wl wl) + 2 (the
                      quotient) = 5 u and 2 e_wl / wl.   D = A - B: e_A + e_B + u |D|.   coef = ((1000 D) k) / nel, times ls: the
                      product 1, k and ls exact (powers of two or 1), the quotient 2:  |1000 k ls / nel| e_D + 3 u |coef|
               rec    1000 (sum e_term + (n - 1) u sum |term|) + u |rec|;   wd exact;   total  e_rec + u |total|
               agg    e_wl when training, else bit-identical
               L2     m: u |m|;  coef: 1000.f/255.f (1), the quotient (2) = 3 u |coef|;  1000 m: 2 u;  1000 m / 255: 4 u, + u |total|
    optimizer  g'     u (|g gs| + |wd w| + |g'|) + wd e_w  (gs = grad_scale / S is a power of two in every test: exact)
               norm2  a chunk sum is at most 16 roundings deep on a sum of squares (the square 1, two trips of a thread 3, the
                      workgroup tree 8, spare 4):  e = sum 2 |g'| e_g' + 17 u norm2  (the 17th: the cast of the f64 total)
               factor relative e_f = e_norm2 / (2 norm2) + 4 u (sqrtf, the quotient) where sqrt(norm2) (1 + e) >= clip, else 0
               gc     factor e_g' + |gc| e_f + u |gc|
               m      b1 e_m + (1 - b1) e_gc + u (|b1 m| + |(1 - b1) gc| + |m'|)        (1 - beta is exact in f32 for beta >= 1/2)
               v      b2 e_v + (1 - b2) 2 |gc| e_gc + u (b2 v + 2 (1 - b2) gc^2 + v')     (adagrad: b2 = 1 and (1 - b2) = 1)
               adam   den = sqrt(v) + eps:  e_den = e_v / (2 sqrt v) + 2 u sqrt v + u den  (0 where v == 0 exactly: then m == 0 too);
                      upd = lr_t m / den:  lr_t (e_m / den + |m| e_den / den^2) + 7 u |upd|  (lr_t within 2 ulp = 4 u, the
                      product 1, the quotient 2);  w': e_w + e_upd + u |w'|
               adadelta  num = sqrt(m + eps): (e_m + u (m + eps)) / (2 num) + 2 u num, den = sqrt(v + eps) alike;  q = num / den:
                      e_num / den + num e_den / den^2 + 2 u q;  upd = q gc: |gc| e_q + q e_gc + u |upd|;  w': e_w + lr e_upd + 2 u lr |upd| + u |w'|
               adagrad   s = sqrt(v): e_v / (2 s) + 2 u s;  upd = lr gc / s: lr (e_gc / s + |gc| e_s / s^2) + 4 u |upd|;  w' as above
               left out  an element whose e_den exceeds den / 4 (Adam: sqrt(v) not far above its own error, where the quotient's
                      conditioning defeats a first-order count) or whose e_gc exceeds |gc| / 4 while gc != 0; at most 1 % of a case
    lr_state   two f32 ulps (the f64 result and its cast, and a pow that differs from numpy's in the last place)
"""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bn_reference import F64, STORAGE, STORAGE_IDS, U, exact_in_f32, f32, half_ulp, ratio, store, stored_bits, violations, widen  # noqa: E402,F401

C01 = float(np.float32(0.01))
SLACK = 1.0 + 2.0 ** -10
SSE_BLOCKS, THREADS = 512, 256
NORM2_SANE = 1e30                # IMM_NORM2_SANE of loss_optim.hip
LOSS_PERCEPTUAL, LOSS_L2 = 0, 1
LIMIT = float(2 ** 24)
BF16, F16, F32T = STORAGE
_cache = {}


def clear_cache():
    _cache.clear()


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def r32(x):
    """The f32 value nearest x, as a python float (what a kernel is handed for a host constant)."""
    return float(np.float32(x))


# ----------------------------------------------------------------------------------------------
# error sums
# ----------------------------------------------------------------------------------------------
def pick(mask, S, s):
    """The mask the loss reads at a feature of side s: mask[b, y r, x r], r = S / s."""
    r = S // s
    return mask[:, ::r, ::r][:, :s, :s]


def sse_terms(a, b, mask, S, s, l1):
    """The per-pixel terms mask * sum_ch f(a - b), shape [B, s, s]."""
    d = a - b
    t = (np.abs(d) if l1 else d * d).sum(-1)
    return t if mask is None else t * pick(mask, S, s)


def sse(a, b, mask, S, s, l1):
    return float(sse_terms(a, b, mask, S, s, l1).sum())


def block_abs_sums(t, per_item=1):
    """Sum of |t| per workgroup of a grid-stride launch of SSE_BLOCKS x THREADS over t.size / per_item items."""
    t = np.abs(np.asarray(t, F64)).reshape(-1, per_item).sum(1)
    n = SSE_BLOCKS * THREADS
    t = np.concatenate([t, np.zeros(-t.size % n)])
    return t.reshape(-1, SSE_BLOCKS, THREADS).sum((0, 2))


# ----------------------------------------------------------------------------------------------
# finalize
# ----------------------------------------------------------------------------------------------
def finalize(partial, nel, agg, training, wd, l1, mode, S=None):
    """-> (out[3 n + 3], new agg), f64.  partial [n, SSE_BLOCKS] f32, nel / agg [n] f32, wd an f32 value or None, S the loss scale."""
    partial = np.asarray(partial)
    assert partial.dtype == np.float32 and partial.ndim == 2
    n = partial.shape[0]
    nel, agg = np.asarray(nel, F64), np.asarray(agg, F64)
    ls, wd = (1.0 if S is None else float(S)), (0.0 if wd is None else float(wd))
    m = partial.astype(F64).sum(1) / nel
    out = np.zeros(3 * n + 3)
    if mode == LOSS_L2:
        assert n == 1 and not l1
        out[:] = [m[0], m[0], ls * (1000.0 / 255.0) * 2.0 / nel[0], 1000.0 * m[0], wd, 1000.0 * m[0] / 255.0 + wd]
        return out, agg.copy()
    wl = agg + C01 * (m - agg)
    term = m / wl
    out[:n], out[n:2 * n] = term, m
    out[2 * n:3 * n] = ls * 1000.0 * (1.0 / wl - C01 * m / (wl * wl)) * (1.0 if l1 else 2.0) / nel
    out[3 * n] = 1000.0 * term.sum()
    out[3 * n + 1] = wd
    out[3 * n + 2] = out[3 * n] + wd
    return out, (wl if training else agg.copy())


def finalize_bounds(partial, nel, agg, training, wd, l1, mode, S=None):
    """The bounds of finalize()'s (out, agg), as the docstring derives them."""
    out, _ = finalize(partial, nel, agg, training, wd, l1, mode, S)
    n = np.asarray(partial).shape[0]
    nel, agg = np.asarray(nel, F64), np.asarray(agg, F64)
    ls = 1.0 if S is None else float(S)
    b = np.zeros_like(out)
    if mode == LOSS_L2:
        b[:] = [U * abs(out[0]), U * abs(out[1]), 3 * U * abs(out[2]), 2 * U * abs(out[3]), 0.0, 4 * U * abs(out[3] / 255.0) + U * abs(out[5])]
        return b * SLACK, np.zeros(n)
    m = out[n:2 * n]
    wl = agg + C01 * (m - agg)
    e_m = U * np.abs(m)
    e_wl = U * (C01 * np.abs(m) + 2 * C01 * np.abs(m - agg) + np.abs(wl))
    term = m / wl
    e_term = e_m / np.abs(wl) + np.abs(m) * e_wl / wl ** 2 + 2 * U * np.abs(term)
    A, B = 1.0 / wl, C01 * m / (wl * wl)
    e_D = (e_wl / wl ** 2 + 2 * U * np.abs(A)) + np.abs(B) * (5 * U + 2 * e_wl / np.abs(wl)) + U * np.abs(A - B)
    k = 1.0 if l1 else 2.0
    b[:n], b[n:2 * n] = e_term, e_m
    b[2 * n:3 * n] = np.abs(1000.0 * k * ls / nel) * e_D + 3 * U * np.abs(out[2 * n:3 * n])
    b[3 * n] = 1000.0 * (e_term.sum() + (n - 1) * U * np.abs(term).sum()) + U * abs(out[3 * n])
    b[3 * n + 2] = b[3 * n] + U * abs(out[3 * n + 2])
    return b * SLACK, (e_wl * SLACK if training else np.zeros(n))


FINALIZE_NFEAT = [1, 6, 16]


def finalize_exact_table(nfeat):
    """Integer partial rows (times 2^-f) whose f64 sum is exact and whose f32 sum is not, in any order that keeps the two large
    entries apart: row f holds 2^30 at index 37 f, -2^30 at index 37 f + 300 (another lane, another trip) and small integers in
    [1, 3] elsewhere, so the total is the sum of the small ones alone, which f32 loses next to 2^30.  nel = 2^(10 + f)."""
    def build():
        g = np.random.RandomState(900 + nfeat)
        t = g.randint(1, 4, size=(nfeat, SSE_BLOCKS)).astype(F64)
        f = np.arange(nfeat)
        t[f, (37 * f) % SSE_BLOCKS] = 2.0 ** 30
        t[f, (37 * f + 300) % SSE_BLOCKS] = -2.0 ** 30
        t *= 2.0 ** -f[:, None]
        nel = 2.0 ** (10 + f)
        return t.astype(np.float32), nel.astype(np.float32)
    return cached(('fin_exact', nfeat), build)


def f32_sums(row):
    """Three f32 summation orders of one partial row: index order, the kernel's lanes (eight per lane, then a butterfly) and pairwise."""
    x = np.asarray(row, np.float32)
    seq = np.float32(0)
    for v in x:
        seq = np.float32(seq + v)
    lanes = x.reshape(-1, 64)
    acc = np.zeros(64, np.float32)
    for i in range(lanes.shape[0]):
        acc = (acc + lanes[i]).astype(np.float32)
    o = 32
    while o >= 1:
        acc = (acc + acc[np.arange(64) ^ o]).astype(np.float32)
        o >>= 1
    pw = x.copy()
    while pw.size > 1:
        pw = (pw[0::2] + pw[1::2]).astype(np.float32)
    return float(seq), float(acc[0]), float(pw[0])


def finalize_real_case(nfeat, seed=0):
    """Partials of a realistic step: rows of different magnitude (an image term near 1e7, features near 1e2 .. 1e4), nel, agg, wd."""
    g = np.random.RandomState(77 + nfeat + seed)
    mag = 10.0 ** g.uniform(-1, 5, size=nfeat)
    part = (mag[:, None] * g.uniform(0.5, 1.5, size=(nfeat, SSE_BLOCKS))).astype(np.float32)
    nel = np.asarray([float(2 * 16 * 16 * 8 * (f + 1)) for f in range(nfeat)], np.float32)
    agg = (part.astype(F64).sum(1) / nel * g.uniform(0.3, 3.0, size=nfeat)).astype(np.float32)
    return part, nel, agg, np.float32(0.37)


# ----------------------------------------------------------------------------------------------
# gradient injection
# ----------------------------------------------------------------------------------------------
def tap_grad(d_in, ap, ag, mask, S, ck, relu, l1):
    s = ap.shape[1]
    e = ap - ag
    if l1:
        e = np.sign(e)
    cm = ck * (1.0 if mask is None else pick(mask, S, s)[..., None])
    v = (0.0 if d_in is None else d_in) + cm * e
    if relu:
        v = np.where(ap > 0, v, 0.0)
    return v + 0.0                                                           # every zero the kernel stores is +0


def window_argmax(ap):
    """[B, h/2, w/2, c]: the index 0..3 of the FIRST maximum of each 2x2 window in the order (0,0), (0,1), (1,0), (1,1)."""
    B, h, wd, c = ap.shape
    w = ap.reshape(B, h // 2, 2, wd // 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(B, h // 2, wd // 2, 4, c)
    return w.argmax(3), w                                                    # numpy: the first occurrence


def unpool(dpool, ap):
    """max_pool2d's backward: dpool routed to the first maximum of each window."""
    B, h, wd, c = ap.shape
    am, _w = window_argmax(ap)
    hot = np.arange(4)[None, None, None, :, None] == am[:, :, :, None, :]
    up = np.where(hot, dpool[:, :, :, None, :], 0.0)
    return up.reshape(B, h // 2, wd // 2, 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(B, h, wd, c)


def unpool_tap_grad(dpool, ap, ag, mask, S, ck):
    return tap_grad(unpool(dpool, ap), ap, ag, mask, S, ck, True, False)


def image_loss_grad(gt, pred, mask, ck, l1, lddp):
    """gt, pred [npix, 3], mask [npix] or None -> [npix, lddp]; (coef mask) e keeps the sign of a zero product, as the kernel does."""
    e = pred - gt
    if l1:
        e = np.sign(e)
    cm = ck * (np.ones(gt.shape[0]) if mask is None else mask)
    out = np.zeros((gt.shape[0], lddp))
    out[:, :3] = cm[:, None] * e
    return out


# ----------------------------------------------------------------------------------------------
# optimizer
# ----------------------------------------------------------------------------------------------
CHUNK = 2048
ADAM, ADADELTA, ADAGRAD = 0, 1, 2


def chunks(sizes, chunk=CHUNK):
    """ops.SegmentTable's layout: offsets, and per chunk (segment, begin, end), and each segment's first chunk."""
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    seg, b0, b1, first = [], [], [], [0]
    for s, n in enumerate(sizes):
        for k in range(0, int(n), chunk):
            seg.append(s)
            b0.append(offs[s] + k)
            b1.append(offs[s] + min(int(n), k + chunk))
        first.append(len(seg))
    return SimpleNamespace(offsets=offs, seg=np.asarray(seg), begin=np.asarray(b0), end=np.asarray(b1), first=np.asarray(first),
                           nblk=len(seg), nseg=len(sizes), total=int(offs[-1]))


def hparams(**kw):
    """The hyper-parameters as the kernel holds them (f32 values, widened)."""
    d = dict(lr_start=1e-3, lr_decay=0.95, lr_step=100000, lr_multiple=1.0, beta1=0.9, beta2=0.999, eps=1e-8, clip=1.0,
             grad_scale=1.0, optim=ADAM, scale_growth_interval=0, scale_max=0.0)
    d.update(kw)
    hp = SimpleNamespace(**{k: (v if k in ('lr_step', 'optim', 'scale_growth_interval') else r32(v)) for k, v in d.items()})
    assert hp.beta1 >= 0.5 and hp.beta2 >= 0.5, '1 - beta must be exact in f32'
    return hp


def learning_rate(hp, gs, t):
    """-> (lr_t, lr) of the step that starts at global_step gs with Adam's count t (the kernel uses t + 1)."""
    lr = hp.lr_multiple * hp.lr_start * hp.lr_decay ** (gs // hp.lr_step)
    return lr * math.sqrt(1.0 - hp.beta2 ** (t + 1)) / (1.0 - hp.beta1 ** (t + 1)), lr


def per_seg(tab, x):
    return np.repeat(np.asarray(x, F64), np.diff(tab.offsets))


def prepare(g, w, wd, grad_scale, S, tab):
    """-> (g' , chunk sums of g'^2).  wd per segment; S the loss scale or None."""
    gs = grad_scale * (1.0 / S if S is not None else 1.0)
    gp = g * gs + per_seg(tab, wd) * w
    return gp, np.add.reduceat(gp * gp, tab.begin)


def norms(tab, blk_partial):
    """Per tensor: the f64 sum of its chunk sums."""
    return np.add.reduceat(np.asarray(blk_partial, F64), tab.first[:-1])


def clip_factor(norm2, clip):
    n2 = np.asarray(norm2, F64)
    return clip / np.maximum(np.sqrt(n2), clip) if clip > 0 else np.ones_like(n2)


def adam_one(hp, lr_t, lr, g, m, v, w):
    m = hp.beta1 * m + (1.0 - hp.beta1) * g
    v = hp.beta2 * v + (1.0 - hp.beta2) * g * g
    return m, v, w - lr_t * m / (np.sqrt(v) + hp.eps)


def adadelta_one(hp, lr_t, lr, g, m, v, w):
    v = hp.beta1 * v + (1.0 - hp.beta1) * g * g
    u = np.sqrt(m + hp.eps) / np.sqrt(v + hp.eps) * g
    return hp.beta1 * m + (1.0 - hp.beta1) * u * u, v, w - lr * u


def adagrad_one(hp, lr_t, lr, g, m, v, w):
    v = v + g * g
    return m, v, w - lr * g / np.sqrt(v)


ONE = {ADAM: adam_one, ADADELTA: adadelta_one, ADAGRAD: adagrad_one}


def weight_decay_loss(w, wd, tab):
    """-> (per-chunk 0.5 wd sum w^2, their total)."""
    p = 0.5 * np.asarray(wd, F64)[tab.seg] * np.add.reduceat(w * w, tab.begin)
    return p, float(p.sum())


def step(hp, tab, wd, g, w, m, v, gs, t, S=None, err=None):
    """One imm_clip_adam_step (no skip) in f64 with the bounds of the docstring.  err: the (e_w, e_m, e_v) its inputs carry."""
    z = np.zeros_like(w)
    e_w0, e_m0, e_v0 = (z, z, z) if err is None else err
    wdv = per_seg(tab, wd)
    scale = hp.grad_scale * (1.0 / S if S is not None else 1.0)
    r = SimpleNamespace()
    r.grads, r.blk_partial = prepare(g, w, wd, hp.grad_scale, S, tab)
    r.norm2 = norms(tab, r.blk_partial)
    r.factor = clip_factor(r.norm2, hp.clip)
    r.lr_t, r.lr = learning_rate(hp, gs, t)
    r.e_grads = U * (np.abs(g * scale) + np.abs(wdv * w) + np.abs(r.grads)) + wdv * e_w0
    sq = np.add.reduceat(2 * np.abs(r.grads) * r.e_grads, tab.begin)
    r.e_blk = sq + 16 * U * r.blk_partial
    r.e_norm2 = np.add.reduceat(sq, tab.first[:-1]) + 17 * U * r.norm2
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(r.norm2 > 0, r.e_norm2 / (2 * r.norm2), 0.0)
    e_f = np.where((hp.clip > 0) & (np.sqrt(r.norm2) * (1 + rel) >= hp.clip), rel + 4 * U, 0.0)
    gc = r.grads * per_seg(tab, r.factor)
    e_gc = per_seg(tab, r.factor) * r.e_grads + np.abs(gc) * per_seg(tab, e_f) + U * np.abs(gc)
    r.gc = gc
    r.m, r.v, r.w = ONE[hp.optim](hp, r.lr_t, r.lr, gc, m, v, w)
    b1, b2 = hp.beta1, hp.beta2
    with np.errstate(divide='ignore', invalid='ignore'):
        if hp.optim == ADAM:
            r.e_m = b1 * e_m0 + (1 - b1) * e_gc + U * (np.abs(b1 * m) + np.abs((1 - b1) * gc) + np.abs(r.m))
            r.e_v = b2 * e_v0 + (1 - b2) * 2 * np.abs(gc) * e_gc + U * (b2 * v + 2 * (1 - b2) * gc * gc + r.v)
            sv = np.sqrt(r.v)
            den = sv + hp.eps
            e_den = np.where(r.v > 0, r.e_v / (2 * sv), 0.0) + 2 * U * sv + U * den
            upd = r.lr_t * r.m / den
            e_upd = r.lr_t * (r.e_m / den + np.abs(r.m) * e_den / den ** 2) + 7 * U * np.abs(upd)
            r.left_out = e_den > den / 4
        elif hp.optim == ADADELTA:
            r.e_v = b1 * e_v0 + (1 - b1) * 2 * np.abs(gc) * e_gc + U * (b1 * v + 2 * (1 - b1) * gc * gc + r.v)
            num, den = np.sqrt(m + hp.eps), np.sqrt(r.v + hp.eps)
            e_num = (e_m0 + U * (m + hp.eps)) / (2 * num) + 2 * U * num
            e_den = (r.e_v + U * (r.v + hp.eps)) / (2 * den) + 2 * U * den
            q = num / den
            e_q = e_num / den + num * e_den / den ** 2 + 2 * U * q
            uu = q * gc
            e_uu = np.abs(gc) * e_q + q * e_gc + U * np.abs(uu)
            r.e_m = b1 * e_m0 + (1 - b1) * 2 * np.abs(uu) * e_uu + U * (b1 * m + 2 * (1 - b1) * uu * uu + r.m)
            e_upd = r.lr * e_uu + 2 * U * np.abs(r.lr * uu)
            r.left_out = e_den > den / 4
        else:
            r.e_m = e_m0
            r.e_v = e_v0 + 2 * np.abs(gc) * e_gc + U * (gc * gc + r.v)
            s = np.sqrt(r.v)
            e_s = r.e_v / (2 * s) + 2 * U * s
            upd = r.lr * gc / s
            e_upd = r.lr * (e_gc / s + np.abs(gc) * e_s / s ** 2) + 4 * U * np.abs(upd)
            r.left_out = e_s > s / 4
        r.left_out = r.left_out | ((gc != 0) & (e_gc > np.abs(gc) / 4))
    r.e_w = e_w0 + e_upd + U * np.abs(r.w)
    for k in ('e_grads', 'e_blk', 'e_norm2', 'e_m', 'e_v', 'e_w'):
        setattr(r, k, getattr(r, k) * SLACK)
    return r


def ulp32(x):
    x = np.abs(np.asarray(x, F64))
    return 2.0 ** (np.floor(np.log2(np.maximum(x, 2.0 ** -126))) - 23)


# ----------------------------------------------------------------------------------------------
# exact data
# ----------------------------------------------------------------------------------------------
def ints(g, shape, lo, hi):
    return g.randint(lo, hi + 1, size=shape).astype(F64)


SSE_B, SSE_S = 3, 64
SSE_FEATS = [(s, c) for s in (64, 32, 16, 8) for c in (8, 136)]               # r = 1, 2, 4, 8; one vector per pixel and 17
IMG_B, IMG_S = 7, 256                                                         # 458 752 pixels > 3 * 512 * 256
IMG_LD = [(3, 16, False), (4, 4, False), (4, 4, True), (3, 8, False)]         # lda, ldb, both operands start one float into a buffer
IMG_IDS = ['3_16', '4_4_float4', '4_4_misaligned', '3_8']
SMALL_C = [(1, 1, 8), (5, 5, 8), (5, 8, 5)]                                   # c, lda, ldb on 2 x 8 x 8 pixels


def sse_case():
    """Integer features in [-3, 3] at every (s, c) of SSE_FEATS and an integer mask in [0, 3] that differs from sample to sample."""
    def build():
        g = np.random.RandomState(41)
        e = SimpleNamespace(mask=ints(g, (SSE_B, SSE_S, SSE_S), 0, 3), feats=[])
        for s, c in SSE_FEATS:
            e.feats.append((ints(g, (SSE_B, s, s, c), -3, 3), ints(g, (SSE_B, s, s, c), -3, 3)))
        return e
    return cached('sse', build)


def image_case(B=IMG_B, S=IMG_S, c=3):
    """Integer pixels and mask in [0, 3]."""
    def build():
        g = np.random.RandomState(43 + c + B)
        return SimpleNamespace(a=ints(g, (B, S, S, c), 0, 3), b=ints(g, (B, S, S, c), 0, 3), mask=ints(g, (B, S, S), 0, 3))
    return cached(('img', B, S, c), build)


# gradient injection: incoming gradients whose sum with coef mask e the 16-bit store rounds (integers every type holds exactly)
TAP_B, TAP_S, TAP_C = 3, 8, 24
D_AMP = {BF16: 128, F16: 2000, F32T: 2000}
TAP_COEF = 0.375
TAP_MASK_SIDE = [None, 8, 16, 64]                                             # no mask, r = 1, 2, 8
IMG_COEF = {BF16: 0.375, F16: 4.125, F32T: 4.125}


def tap_case(dt):
    def build():
        g = np.random.RandomState(51 + D_AMP[dt])
        shape = (TAP_B, TAP_S, TAP_S, TAP_C)
        e = SimpleNamespace(ap=ints(g, shape, -3, 3), ag=ints(g, shape, -3, 3), d=ints(g, shape, -D_AMP[dt], D_AMP[dt]))
        e.masks = {S: ints(g, (TAP_B, S, S), 0, 3) for S in TAP_MASK_SIDE if S}
        return e
    return cached(('tap', dt), build)


UNPOOL_B, UNPOOL_S, UNPOOL_C = 3, 16, 24
UNPOOL_COEF = {BF16: 37.125, F16: 0.375, F32T: 0.375}                         # three pixels in four get no dpool: bf16 must round coef mask e alone


def unpool_case(dt):
    def build():
        g = np.random.RandomState(61 + D_AMP[dt])
        shape = (UNPOOL_B, UNPOOL_S, UNPOOL_S, UNPOOL_C)
        e = SimpleNamespace(ap=ints(g, shape, -2, 3), ag=ints(g, shape, -3, 3))
        e.dpool = ints(g, (UNPOOL_B, UNPOOL_S // 2, UNPOOL_S // 2, UNPOOL_C), -D_AMP[dt], D_AMP[dt])
        e.masks = {S: ints(g, (UNPOOL_B, S, S), 0, 3) for S in (16, 32)}
        return e
    return cached(('unpool', dt), build)


IMGRAD_B, IMGRAD_S = 3, 20                                                    # 1200 pixels: more than one workgroup at lddp 16


def imgrad_case():
    def build():
        g = np.random.RandomState(71)
        n = IMGRAD_B * IMGRAD_S * IMGRAD_S
        return SimpleNamespace(gt=ints(g, (n, 3), 0, 255), pred=ints(g, (n, 3), 0, 255), mask=ints(g, (n,), 0, 3))
    return cached('imgrad', build)


# the one exact optimizer step
EXACT_SIZES = [1, 2049, 2, 3, 5, 2047, 2048, 4099]
EXACT_WD = [0.0, 0.25, 0.0, 0.25, 0.0, 0.25, 0.0, 0.25]
EXACT_HP = dict(beta1=0.5, beta2=0.75, grad_scale=0.5, clip=256.0, eps=1e-8, lr_start=1e-3)


def exact_opt_case():
    """g integers in [-4, 4] (times grad_scale 1/2), w = k/4 with |w| <= 8 and wd = 1/4 (|wd w| <= 2: the size of |g grad_scale|), m
    and v quarters.  The small tensors carry the clipped norms: 512 (factor 1/2), (0, 1024) (1/4) and four times 256 and a 0 (1/2);
    the rest stay below clip = 256 (factor exactly 1)."""
    def build():
        g = np.random.RandomState(81)
        tab = chunks(EXACT_SIZES)
        e = SimpleNamespace(tab=tab, wd=np.asarray(EXACT_WD), hp=hparams(**EXACT_HP))
        e.g, e.w = ints(g, tab.total, -4, 4), ints(g, tab.total, -32, 32) / 4
        e.m, e.v = ints(g, tab.total, -8, 8) / 4, ints(g, tab.total, 0, 16) / 4
        o = tab.offsets
        e.g[o[0]] = 1024.0                                                   # g' = 512
        e.g[o[2]:o[3]] = [0.0, 2048.0]                                       # g' = (0, 1024)
        e.g[o[4]:o[5]] = [512.0, 512.0, 0.0, 512.0, 512.0]                  # g' = 256 four times: norm 512
        return e
    return cached('opt_exact', build)


# the default prologue: two tensors of more than 256 chunks, small ones before, between and after
PRO_SIZES = [3, 257 * CHUNK + 5, 7, 5, 300 * CHUNK, 2, 1]
PRO_WD = [0.0, 0.25, 0.0, 0.0, 0.0, 0.25, 0.0]
PRO_SCALE = [2.0 ** 6, 2.0 ** -12, 1.0, 1.0, 1.0, 2.0 ** -20, 2.0 ** 10]      # per-tensor gradient scale: norms over many orders
PRO_HP = dict(beta1=0.5, beta2=0.75, grad_scale=1.0, clip=4.0, eps=1e-8, lr_start=1e-3)
PRO_ZERO, PRO_AT_CLIP = 3, 2                                                  # the all-zero tensor; the tensor whose norm == clip


def prologue_case():
    def build():
        g = np.random.RandomState(91)
        tab = chunks(PRO_SIZES)
        e = SimpleNamespace(tab=tab, wd=np.asarray(PRO_WD), hp=hparams(**PRO_HP))
        e.g = ints(g, tab.total, -3, 3) * per_seg(tab, PRO_SCALE)
        e.w = ints(g, tab.total, -32, 32) / 4 * per_seg(tab, [1, 2.0 ** -12, 1, 1, 1, 2.0 ** -20, 1])
        o = tab.offsets
        e.g[o[PRO_ZERO]:o[PRO_ZERO + 1]] = 0.0
        e.g[o[PRO_AT_CLIP]:o[PRO_AT_CLIP + 1]] = [0.0, 0.0, 4.0, 0.0, 0.0, 0.0, 0.0]
        e.m = e.v = np.zeros(tab.total)
        return e
    return cached('prologue', build)


# three steps on real data
REAL_SIZES = [4099, 5, 2048, 1, 300, 2049]
REAL_WD = [1e-2, 0.0, 1e-2, 0.0, 0.0, 1e-2]
REAL_G = [3.0, 1e-3, 0.05, 2.0, 1e-3, 1e-3]
REAL_RUNS = {'adam': dict(optim=ADAM, clip=1.0), 'adam_noclip': dict(optim=ADAM, clip=0.0),
             'adadelta': dict(optim=ADADELTA, clip=1.0, beta1=0.95, eps=1e-6, lr_start=1e-2),
             'adagrad': dict(optim=ADAGRAD, clip=1.0, lr_start=1e-2)}
LEFT_OUT_CAP = 0.01


def real_opt_case(name):
    """randn gradients (the SUM over two towers: grad_scale 1/2) of per-tensor size REAL_G, weights 0.3 randn, wd 1e-2 on the
    filters; three steps of the f64 reference with the bounds carried from step to step."""
    def build():
        g = np.random.RandomState(101)
        tab = chunks(REAL_SIZES)
        e = SimpleNamespace(tab=tab, wd=f32(REAL_WD).astype(F64), hp=hparams(grad_scale=0.5, **REAL_RUNS[name]))
        e.g = f32(2.0 * g.standard_normal(tab.total) * per_seg(tab, REAL_G)).astype(F64)
        e.w0 = f32(0.3 * g.standard_normal(tab.total)).astype(F64)
        e.m0 = np.zeros(tab.total)
        e.v0 = np.full(tab.total, r32(0.1)) if e.hp.optim == ADAGRAD else np.zeros(tab.total)
        e.steps, w, m, v, err = [], e.w0, e.m0, e.v0, None
        for it in range(3):
            r = step(e.hp, tab, e.wd, e.g, w, m, v, it, it, err=err)
            e.steps.append(r)
            w, m, v, err = r.w, r.m, r.v, (r.e_w, r.e_m, r.e_v)
        return e
    return cached(('opt_real', name), build)
