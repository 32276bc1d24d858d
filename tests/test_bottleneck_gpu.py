"""The landmark bottleneck and the pose head of imm_amd/csrc/bottleneck.hip on a real MI355X: soft-argmax, Gaussian maps, their backward,
the fused pose head both ways and the two render-only kernels.

A. Exact, bit for bit.  Heat-maps of integers whose softmax is exactly {1/n on the winners, 0 elsewhere} (bottleneck_reference.exact_heat):
   mu, py, px equal predicted bits, with landmarks on the first and last row, at 0 and off the grid; a common offset of 8192 changes no bit
   (a softmax without its max-subtraction gives NaN); a saturated softmax and a zero dgauss pass no gradient, the kink pixel included; the
   pose head's convolution on integers, and its data gradient through selector filters, against the dheat the same launch stored.
B. Real data against the numpy f64 restatement within bounds counted from roundings (the table in bottleneck_reference's docstring), by the
   window rule: landmarks up to the image edge, K off the kernel's 10 landmarks per pass, h != w, s != h, f32 storage, LDS above 64 KB.
   Each bounded test prints its largest err/bound (run with -s); nothing is left out of any comparison.
C. Every limit the entry points refuse raises and leaves the outputs untouched.

Every device tensor is a guarded buffer (tests/guarded.py); an input wider than its payload carries NaN there.  What the data must
satisfy for all this to mean anything is asserted without a GPU in tests/test_bottleneck_cpu.py.
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
import bottleneck_reference as R                                            # noqa: E402
from exact_data import exact_equal                                          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN = float('nan')
F32 = torch.float32
BF16, F16 = torch.bfloat16, torch.float16
DT16 = pytest.mark.parametrize('dt', [BF16, F16], ids=['bf16', 'f16'])
MODE = pytest.mark.parametrize('mode', R.MODES)
T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731
T32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))   # noqa: E731
_INT = {2: torch.int16, 4: torch.int32}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from imm_amd import ops as _ops
    torch.cuda.set_device(0)
    return _ops


@pytest.fixture(scope='module')
def lib_error():
    from imm_amd import _lib
    return _lib.ImmHipError


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
    return guarded.inp(t.contiguous(), DEV, depth=2)


def wide(t, ld, rows=None):
    """A kernel INPUT [..., c] embedded in [..., ld] on the device; the columns [c, ld) hold NaN (and so do rows past the payload)."""
    c = t.shape[-1]
    shape = list(t.shape[:-1]) + [ld]
    if rows is not None:
        shape[0] = rows
    o = torch.full(shape, NAN, dtype=t.dtype)
    o[:t.shape[0], ..., :c] = t
    return guarded.inp(o, DEV, depth=2)


def gout(shape, dt, fill=None):
    return guarded.out(shape, dt, DEV, fill=fill, what=guarded._caller(1))


def same_bits(a, b, what):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ai, bi = a.view(_INT[a.element_size()]), b.view(_INT[b.element_size()])
    n = int((ai != bi).sum())
    assert n == 0, '%s: %d/%d elements differ in bits' % (what, n, ai.numel())


def held(got, ref, bound, dt, what):
    """No element outside its window (bottleneck_reference.window); returns err/bound for the report."""
    got = R.widen(got)
    ref, bound = np.broadcast_arrays(np.asarray(ref, np.float64), np.asarray(bound, np.float64))
    bad = R.window(got, ref, bound, dt)
    r = R.ratio(got, ref, bound, dt)
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError('%s: %d/%d elements outside their window (%d not finite), largest err/bound %.3g, first at %s got %r ref %r bound %.3g' % (
            what, int(bad.sum()), bad.size, int((~np.isfinite(got)).sum()), r, i, float(got[i]), float(ref[i]), float(bound[i])))
    return r


def bits(dt):
    """The 16-bit figures sit near 1 by construction (the store's own half ulp is most of the window); the f32 ones show the arithmetic."""
    return 'f32' if dt == F32 else '16-bit'


def report(name, **ratios):
    print('\n%s: largest err/bound %s; left out 0' % (name, ', '.join('%s %.3f' % kv for kv in ratios.items())))


# ---- launches ---------------------------------------------------------------------------------
def run_fwd(ops, heat, s, inv_std, mode, dt, maps=True):
    """imm_softargmax_gauss_fwd on heat [B, h, w, K] (numpy, exact in f32) with ldh > K and ldg > K."""
    B, h, w, K = heat.shape
    ldh, ldg = K + 3, K + 5
    assert R.exact_in_f32(heat)
    o = SimpleNamespace(mu=gout((B, K, 2), F32), py=gout((B, h, K), F32), px=gout((B, w, K), F32), g=None)
    joint = gout((B, s, s, ldg), dt) if maps else None
    ops.softargmax_gauss_fwd(wide(T32(heat), ldh), ldh, B, h, w, K, inv_std, s, o.mu, o.py, o.px, joint, ldg, dt, mode)
    torch.cuda.synchronize()
    if maps:
        assert untouched(joint[..., K:]), 'imm_softargmax_gauss_fwd wrote columns [K, ldg)'
        o.g = joint[..., :K]
    return o


def pack_fwd(W, dt, C, K):
    """The forward filter as the kernel reads it: wt[n][c] = W[c][n], 64 rows, rows [K, 16 ceil(K / 16)) zero (they are multiplied and
    dropped), everything the kernel must not read NaN."""
    wt = torch.full((64, C + 32), NAN, dtype=dt)
    wt[:(K + 15) // 16 * 16, :C] = 0
    wt[:K, :C] = R.store(np.asarray(W).T, dt)
    return guarded.inp(wt, DEV, depth=2)


def run_head_fwd(ops, feat, W, bias, s, inv_std, mode, dt, h, w, maps=True):
    """imm_pose_head_fwd: feat [B, h, w, C] and W [C, K] exact in dt, bias [K] exact in f32; ldf > C, ldh > K, ldg > K."""
    B, C, K = feat.shape[0], feat.shape[-1], W.shape[1]
    ldf, ldh, ldg = C + 8, K + 3, K + 5
    ft = R.store(feat, dt)
    assert torch.equal(ft.double(), T64(feat)) and torch.equal(R.store(W, dt).double(), T64(W)), 'operands not representable in %s' % dt
    o = SimpleNamespace(mu=gout((B, K, 2), F32), py=gout((B, h, K), F32), px=gout((B, w, K), F32), g=None, heat=None)
    heat = gout((B, h, w, ldh), F32)
    joint = gout((B, s, s, ldg), dt) if maps else None
    ops.pose_head_fwd(wide(ft, ldf), ldf, C, pack_fwd(W, dt, C, K), dev(T32(bias)), B, h, w, K, inv_std, s, heat, ldh, o.mu, o.py, o.px,
                      joint, ldg, dt, mode)
    torch.cuda.synchronize()
    assert untouched(heat[..., K:]), 'imm_pose_head_fwd wrote heat columns [K, ldh)'
    o.heat = heat[..., :K]
    if maps:
        assert untouched(joint[..., K:]), 'imm_pose_head_fwd wrote map columns [K, ldg)'
        o.g = joint[..., :K]
    return o


def run_bwd(ops, dg, mu, py, px, h, w, inv_std, mode, lddh):
    """imm_softargmax_gauss_bwd; dg [B, s, s, K] of the storage type (ldg > K), mu / py / px f32 device tensors.  -> dheat [B, h, w, lddh]."""
    B, s, K = dg.shape[0], dg.shape[1], dg.shape[3]
    ldg = K + 5
    dheat = gout((B, h, w, lddh), dg.dtype)
    ops.softargmax_gauss_bwd(wide(dg, ldg), ldg, B, h, w, K, inv_std, s, mu, py, px, dheat, lddh, mode)
    torch.cuda.synchronize()
    return dheat


def run_head_bwd(ops, dg, mu, py, px, h, w, inv_std, mode, lddh, wtd64, C):
    """imm_pose_head_bwd; wtd64 [C][lddh] exact in the storage type; lddf > C, the filter rows wider than lddh."""
    B, s, K, dt = dg.shape[0], dg.shape[1], dg.shape[3], dg.dtype
    ldg, lddf = K + 5, C + 4
    wt = R.store(wtd64, dt)
    assert torch.equal(wt.double(), T64(wtd64)) and wtd64.shape == (C, lddh)
    o = SimpleNamespace(dheat=gout((B, h, w, lddh), dt), bias=gout((B, K), F32))
    dfeat = gout((B, h, w, lddf), dt)
    ops.pose_head_bwd(wide(dg, ldg), ldg, B, h, w, K, inv_std, s, mu, py, px, o.dheat, lddh, wide(wt, lddh + 8), C, dfeat, lddf, o.bias, mode)
    torch.cuda.synchronize()
    assert untouched(dfeat[..., C:]), 'imm_pose_head_bwd wrote dfeat columns [C, lddf)'
    o.dfeat = dfeat[..., :C]
    return o


def landmarks(family, B, h, w, K):
    """Host-made inputs of a backward launch: the f64 soft-argmax of a real heat-map, rounded to the f32 the kernel is handed."""
    f = R.forward(R.real_heat(family, B, h, w, K).astype(np.float64))
    mu, py, px = f.mu.astype(np.float32), f.py.astype(np.float32), f.px.astype(np.float32)
    return SimpleNamespace(mu=mu, py=py, px=px, d=(dev(T32(mu)), dev(T32(py)), dev(T32(px))))


def cross_features(e, dt):
    """Features and filter whose 1x1 convolution IS the exact heat-map of sample 0: feat[p = (y, x)][c] = [c == y] + [c == h + x],
    W[c][k] = 256 ([c in Y_k] + [c - h in X_k])."""
    h, w, K = e.h, e.w, e.K
    C = -(-(h + w) // 32) * 32
    feat, W = np.zeros((e.B, h, w, C)), np.zeros((C, K))
    feat[:, np.arange(h), :, np.arange(h)] = 1
    for x in range(w):
        feat[:, :, x, h + x] += 1
    for b, k, Y, X in e.sets:
        if b == 0:
            W[Y, k] += R.P_EXACT
            W[[h + x for x in X], k] += R.P_EXACT
    assert np.array_equal(np.einsum('bhwc,ck->bhwk', feat, W)[0], e.heat[0])
    return feat, W


# ==============================================================================================
# A. exact, bit for bit
# ==============================================================================================
@pytest.mark.parametrize('K', [1, 7, 11, 64])
@pytest.mark.parametrize('h,w', [(16, 16), (5, 12), (32, 16), (1, 7), (4, 4)])
def test_softargmax_exact_and_shift_invariant(ops, h, w, K):
    """A1 + A2: mu, py, px are the predicted bits in every map storage type and through the pose head; + 8192 changes no bit, maps included."""
    e = R.exact_heat(h, w, K)
    s = h if h > 1 else 5
    want = [T32(e.mu), T32(e.py), T32(e.px)]
    for dt in R.STORAGE:
        for mode in (R.MODES if dt == BF16 else ['rot']):
            o, sh = run_fwd(ops, e.heat, s, 10.0, mode, dt), run_fwd(ops, e.heat + R.SHIFT, s, 10.0, mode, dt)
            for r, tag in ((o, ''), (sh, ' + 8192')):
                for got, wnt, name in zip((r.mu, r.py, r.px), want, ('mu', 'py', 'px')):
                    exact_equal(got, wnt, '%s%s %s %s' % (name, tag, mode, dt))
            same_bits(o.g, sh.g, 'maps under the shift %s %s' % (mode, dt))
            assert bool(torch.isfinite(o.g.float()).all())
    if (h * w) % 16 == 0:
        for dt in (BF16, F16):
            feat, W = cross_features(e, dt)
            zero, off = np.zeros(K), np.full(K, float(R.SHIFT))
            o, sh = run_head_fwd(ops, feat, W, zero, s, 10.0, 'rot', dt, h, w), run_head_fwd(ops, feat, W, off, s, 10.0, 'rot', dt, h, w)
            exact_equal(o.heat, T32(np.broadcast_to(e.heat[0], o.heat.shape)), 'pose head: the cross heat-map through the convolution')
            exact_equal(sh.heat, T32(np.broadcast_to(e.heat[0] + R.SHIFT, o.heat.shape)), 'pose head: heat + 8192')
            for r, tag in ((o, ''), (sh, ' + 8192')):
                for got, wnt, name in zip((r.mu, r.py, r.px), want, ('mu', 'py', 'px')):
                    exact_equal(got, wnt[:1].expand(got.shape), 'pose head %s%s %s' % (name, tag, dt))
            same_bits(o.g, sh.g, 'pose head maps under the shift %s' % dt)
            # (not bit for bit against the standalone kernel's maps: the head's 'rot' launch is a compile-time specialisation, and the
            # compiler contracts (dy dy + dx dx) i2 differently there: 2 of 22 528 bf16 values one ulp apart at 32x16x11.  Both lie
            # inside the window.)
            ref, bound = R.render(np.broadcast_to(e.mu[:1], e.mu.shape), s, 10.0, 'rot')
            held(o.g, ref, bound, dt, 'pose head maps %s' % dt)


@MODE
@pytest.mark.parametrize('dt', R.STORAGE, ids=R.STORAGE_IDS)
@pytest.mark.parametrize('h,w,K,s', [(16, 16, 11, 16), (5, 12, 7, 12), (4, 4, 64, 4)])
def test_maps_of_the_exact_landmarks(ops, h, w, K, s, dt, mode):
    """A3: the maps of the exact mu pass the window rule, and the pixel ON a landmark holds the one value the mode defines there."""
    e = R.exact_heat(h, w, K)
    o = run_fwd(ops, e.heat, s, 10.0, mode, dt)
    exact_equal(o.mu, T32(e.mu), 'mu')
    ref, bound = R.render(e.mu, s, 10.0, mode)
    r = held(o.g, ref, bound, dt, 'maps %s' % mode)
    dy, dx = R.offsets(e.mu, s)
    on = (dy == 0)[:, :, None, :] & (dx == 0)[:, None, :, :]
    if h == s and w == s:
        assert on.any(), 'this case must render a pixel that sits on its landmark'
    if on.any():
        v, b = R.on_landmark(10.0, mode)
        got = R.widen(o.g)[on]
        assert not R.window(got, np.full(got.shape, v), np.full(got.shape, b), dt).any(), (mode, got, v)
        if mode == 'rot':
            assert (got == 1.0).all()
    report('maps of exact landmarks %s %s %dx%dx%d' % (mode, dt, h, w, K), maps=r)


@MODE
@pytest.mark.parametrize('h,w,K,s,lddh', [(8, 8, 11, 8, 32), (4, 12, 21, 12, 32), (16, 16, 33, 16, 64)])
def test_a_saturated_softmax_passes_no_gradient(ops, h, w, K, s, lddh, mode):
    """A4: one-hot py and px (every winner's lin - mu is exactly 0, every loser's p is 0) and a dense non-zero dgauss: dheat is zero in
    [.., :K] (either sign) and +0 in the padding; the landmarks sit on render pixels (s equals h or w), the kink included."""
    e = R.one_hot_heat(h, w, K)
    mu, py, px = dev(T32(e.mu)), dev(T32(e.py)), dev(T32(e.px))
    dy, dx = R.offsets(e.mu, s)
    assert (dy == 0).any() or (dx == 0).any()
    for dt in R.STORAGE:
        dg = R.dense_dg(e.B, s, K, dt)
        assert bool((dg != 0).all())
        dheat = run_bwd(ops, dg, mu, py, px, h, w, 10.0, mode, lddh)
        assert float(dheat[..., :K].float().abs().max()) == 0.0, 'standalone %s' % dt
        same_bits(dheat[..., K:], torch.zeros_like(dheat[..., K:]), 'padding of dheat %s' % dt)
        if dt != F32:
            o = run_head_bwd(ops, dg, mu, py, px, h, w, 10.0, mode, lddh, R.selector(32, K, lddh), 32)
            assert float(o.dheat[..., :K].float().abs().max()) == 0.0 and float(o.dfeat.float().abs().max()) == 0.0
            same_bits(o.dheat[..., K:], torch.zeros_like(o.dheat[..., K:]), 'padding of the fused dheat %s' % dt)
            assert float(o.bias.abs().max()) == 0.0


@MODE
def test_a_zero_dgauss_gives_zero_everywhere(ops, mode):
    """A5."""
    B, h, w, K, s, lddh, C = 2, 8, 8, 11, 16, 32, 48
    lm = landmarks('bump', B, h, w, K)
    for dt in R.STORAGE:
        dg = torch.zeros((B, s, s, K), dtype=dt)
        dheat = run_bwd(ops, dg, *lm.d, h, w, 10.0, mode, lddh)
        assert float(dheat[..., :K].float().abs().max()) == 0.0
        same_bits(dheat[..., K:], torch.zeros_like(dheat[..., K:]), 'padding')
        if dt != F32:
            wt = R.widen(R.store(np.random.RandomState(5).standard_normal((C, lddh)), dt))
            wt[:, K:] = 0
            o = run_head_bwd(ops, dg, *lm.d, h, w, 10.0, mode, lddh, wt, C)
            assert float(o.dheat.float().abs().max()) == 0.0 and float(o.dfeat.float().abs().max()) == 0.0 and float(o.bias.abs().max()) == 0.0


HEAD_CONV = [(32, 1, 4, 4), (96, 15, 8, 8), (256, 16, 4, 12), (288, 17, 16, 16), (512, 33, 4, 4), (32, 48, 8, 8), (96, 49, 4, 12),
             (288, 64, 8, 8), (512, 64, 16, 16), (256, 49, 16, 16)]


@DT16
@pytest.mark.parametrize('C,K,h,w', HEAD_CONV)
def test_pose_head_convolution_on_integers(ops, C, K, h, w, dt):
    """A6: integer features, integer and dyadic filter taps, half-integer bias: the stored heat-map is the matmul plus bias bit for bit
    (the second chunk of the contraction at C > 256, a partial chunk, waves without a tile at h w < 256, every K tile count)."""
    B = 2
    feat = R.ints((B, h, w, C), -4, 4, 100 + C + K)
    W = R.ints((C, K), -8, 8, 200 + C + K) / np.where(np.arange(K) % 3 == 1, 4.0, 1.0)
    bias = R.ints((K,), -9, 9, 300 + K) / 2
    ref = np.einsum('bhwc,ck->bhwk', feat, W) + bias
    assert float((np.abs(np.einsum('bhwc,ck->bhwk', np.abs(feat), np.abs(W))) + np.abs(bias)).max()) < 2 ** 22
    o = run_head_fwd(ops, feat, W, bias, 1, 10.0, 'rot', dt, h, w, maps=False)
    exact_equal(o.heat, T32(ref), 'pose head heat C%d K%d %dx%d' % (C, K, h, w))
    f = R.forward_bounds(R.widen(o.heat))
    held(o.mu, f.mu, f.e_mu, F32, 'mu of the integer heat-map')


SELECT = [(16, 3, 32, 2, 8, 8), (48, 11, 32, 2, 4, 12), (112, 21, 32, 3, 8, 8), (128, 33, 64, 2, 8, 8), (144, 10, 64, 2, 4, 4),
          (256, 64, 64, 2, 8, 8), (1040, 7, 32, 2, 4, 4), (1040, 40, 64, 2, 4, 4), (128, 3, 32, 513, 4, 4)]


@DT16
@pytest.mark.parametrize('C,K,lddh,B,h,w', SELECT)
def test_pose_head_data_gradient_on_selector_filters(ops, C, K, lddh, B, h, w, dt):
    """A7: W[c][k] = +-2^e at k = c % K, else 0: dfeat[p][c] is +-2^e times the dheat the same launch stored, exactly.  ysplit 1 (C < 128, and
    batch 513), a share of the channel tiles with no tile (C = 144), the second trip of the n0 loop (C = 1040), both lddh."""
    s = 4 if B > 3 else 16
    lm = landmarks('bump', B, h, w, K)
    sel = R.selector(C, K, lddh)
    o = run_head_bwd(ops, R.dense_dg(B, s, K, dt), *lm.d, h, w, 10.0, 'rot', lddh, sel, C)
    factor = torch.from_numpy(sel[np.arange(C), np.arange(C) % K]).float().to(DEV)
    want = (o.dheat[..., torch.arange(C, device=DEV) % K].float() * factor).to(dt).float() + 0.0     # exact; -0 -> +0: a sum starts from +0
    assert float(o.dheat[..., :K].float().abs().max()) > 0 and bool(torch.isfinite(want).all())
    exact_equal(o.dfeat.float() + 0.0, want, 'dfeat C%d K%d lddh%d B%d' % (C, K, lddh, B))
    same_bits(o.dheat, run_bwd(ops, R.dense_dg(B, s, K, dt), *lm.d, h, w, 10.0, 'rot', lddh), 'fused vs standalone dheat')


# ==============================================================================================
# B. real data within the counted bounds
# ==============================================================================================
FWD_CASES = [(8, 8, 10, 16, 10.0), (5, 12, 1, 5, 3.0), (16, 8, 33, 1, 10.0), (16, 16, 64, 24, 3.0), (4, 12, 10, 16, 3.0)]


def check_fwd(o, heat64, s, inv_std, mode, dt, what):
    f = R.forward_bounds(heat64)
    r = dict(mu=held(o.mu, f.mu, f.e_mu, F32, what + ' mu'), py=held(o.py, f.py, f.e_py, F32, what + ' py'),
             px=held(o.px, f.px, f.e_px, F32, what + ' px'))
    ref, bound = R.render(o.mu.cpu().numpy(), s, inv_std, mode)
    r['maps ' + bits(dt)] = held(o.g, ref, bound, dt, what + ' maps')
    return r


@MODE
@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('h,w,K,s,inv_std', FWD_CASES)
def test_forward_within_bounds(ops, h, w, K, s, inv_std, family, mode):
    """B1: mu, py, px against f64; the maps against the f64 render of the kernel's own mu.  Standalone in three storage types, fused in two
    (the heat-map goes through the convolution as W[c = pixel][k] against one-hot features: what the head stores is f32(W16 + bias))."""
    B = 3 if K < 64 else 2
    if R.fwd_lds(h, w, K) > R.LDS_OPT_IN:
        assert (h, w, K) == (16, 16, 64)
    heat = R.real_heat(family, B, h, w, K)
    worst = {}
    for dt in R.STORAGE:
        o = run_fwd(ops, heat, s, inv_std, mode, dt)
        for k, v in check_fwd(o, heat.astype(np.float64), s, inv_std, mode, dt, 'standalone %s' % dt).items():
            worst[k] = max(worst.get(k, 0.0), v)
    if (h * w) % 16 == 0:
        for dt in (BF16, F16):
            C = -(-h * w // 32) * 32
            feat = np.zeros((1, h * w, C))
            feat[0, np.arange(h * w), np.arange(h * w)] = 1
            W = np.zeros((C, K))
            W[:h * w] = R.widen(R.store(heat[0].reshape(h * w, K), dt))
            bias = np.random.RandomState(K).standard_normal(K).astype(np.float32)
            o = run_head_fwd(ops, np.broadcast_to(feat.reshape(1, h, w, C), (B, h, w, C)).copy(), W, bias, s, inv_std, mode, dt, h, w)
            stored = (W[:h * w].astype(np.float32) + bias).reshape(1, h, w, K)
            exact_equal(o.heat, T32(np.broadcast_to(stored, (B, h, w, K))), 'the heat-map the head stores %s' % dt)
            for k, v in check_fwd(o, R.widen(o.heat), s, inv_std, mode, dt, 'fused %s' % dt).items():
                worst['fused ' + k] = max(worst.get('fused ' + k, 0.0), v)
    report('forward %s %s %dx%dx%d s%d' % (family, mode, h, w, K, s), **worst)


@MODE
@pytest.mark.parametrize('K', [1, 9, 11, 21])
def test_backward_single_pixel_within_bounds(ops, K, mode):
    """B2: one non-zero dgauss per landmark: dmu is one product, whatever the reduction does; what remains is function evaluation."""
    worst = {}
    for (h, w, s, inv_std) in [(8, 8, 16, 10.0), (5, 12, 5, 3.0)]:
        lm = landmarks('bump', 3, h, w, K)
        for dt in R.STORAGE:
            dg = R.single_dg(3, s, K, dt)
            dheat = run_bwd(ops, dg, *lm.d, h, w, inv_std, mode, K + 2)
            r = R.backward(R.widen(dg), lm.mu, lm.py, lm.px, inv_std, mode, single=True)
            assert float(np.abs(r.dheat).max()) > 0
            worst[bits(dt)] = max(worst.get(bits(dt), 0.0), held(dheat[..., :K], r.dheat, r.bound, dt, 'dheat %s %s' % (mode, dt)))
            same_bits(dheat[..., K:], torch.zeros_like(dheat[..., K:]), 'padding of dheat')
    report('backward, single pixel %s K%d' % (mode, K), **worst)


# K, (h, w) standalone, (h, w) fused, s, lddh fused, C
BWD_DENSE = [(1, (8, 8), (8, 8), 5, 32, 32), (9, (16, 8), (4, 12), 16, 32, 48), (10, (5, 12), (16, 16), 16, 32, 256),
             (11, (8, 8), (8, 8), 16, 64, 144), (19, (16, 8), (4, 12), 5, 32, 128), (20, (5, 12), (16, 16), 16, 64, 32),
             (21, (8, 8), (8, 8), 16, 32, 288), (32, (16, 8), (4, 12), 16, 32, 64), (33, (5, 12), (16, 16), 5, 64, 160),
             (64, (8, 8), (8, 8), 16, 64, 1040), (3, (16, 8), (32, 16), 16, 64, 128)]


def check_head_dgrad(o, wtd, K, dt, what):
    """B4: dfeat against the f64 product of the STORED dheat and the filter; the bias partials against its column sums."""
    d16 = R.widen(o.dheat)
    ref, bound, bsum, bbound = R.head_dgrad(d16, wtd, K)
    return held(o.dfeat, ref, bound, dt, what + ' dfeat'), held(o.bias, bsum, bbound, F32, what + ' bias partial')


@MODE
@pytest.mark.parametrize('K,hw_alone,hw_fused,s,lddh,C', BWD_DENSE)
def test_backward_dense_within_bounds(ops, K, hw_alone, hw_fused, s, lddh, C, mode):
    """B3 + B4: the reduction bound, with K on and off the 10 landmarks of a pass; f32 dheat standalone; the fused dheat equals the standalone
    one bit for bit (s s <= 256: one trip either way, the same order); dfeat and the bias partial row from the stored dheat."""
    B, worst = 3, {}
    if hw_fused == (32, 16):
        assert R.bwd_lds(32, 16, K, lddh) > R.LDS_OPT_IN
    inv_std = 3.0 if K % 2 else 10.0
    h, w = hw_alone
    lm = landmarks('bump', B, h, w, K)
    for dt in R.STORAGE:
        dg = R.dense_dg(B, s, K, dt)
        ld = K + 1 if dt != F32 else K
        dheat = run_bwd(ops, dg, *lm.d, h, w, inv_std, mode, ld)
        r = R.backward(R.widen(dg), lm.mu, lm.py, lm.px, inv_std, mode)
        key = 'dheat ' + bits(dt)
        worst[key] = max(worst.get(key, 0.0), held(dheat[..., :K], r.dheat, r.bound, dt, 'standalone dheat %s %s' % (mode, dt)))
        same_bits(dheat[..., K:], torch.zeros_like(dheat[..., K:]), 'padding of dheat')
    h, w = hw_fused
    lm = landmarks('bump', B, h, w, K)
    for dt in (BF16, F16):
        dg = R.dense_dg(B, s, K, dt)
        wtd = R.widen(R.store(0.1 * np.random.RandomState(C + K).standard_normal((C, lddh)), dt))
        wtd[:, K:] = 0
        o = run_head_bwd(ops, dg, *lm.d, h, w, inv_std, mode, lddh, wtd, C)
        r = R.backward(R.widen(dg), lm.mu, lm.py, lm.px, inv_std, mode, nthr=R.PH_BWD_THREADS)
        worst['fused dheat'] = max(worst.get('fused dheat', 0.0), held(o.dheat[..., :K], r.dheat, r.bound, dt, 'fused dheat %s %s' % (mode, dt)))
        same_bits(o.dheat, run_bwd(ops, dg, *lm.d, h, w, inv_std, mode, lddh), 'fused vs standalone dheat %s' % dt)
        a, b = check_head_dgrad(o, wtd, K, dt, 'fused %s %s' % (mode, dt))
        worst['dfeat'], worst['bias'] = max(worst.get('dfeat', 0.0), a), max(worst.get('bias', 0.0), b)
    report('backward, dense %s K%d' % (mode, K), **worst)


@MODE
@pytest.mark.parametrize('h,w,K,s,lddh', [(8, 8, 11, 5, 32), (4, 12, 21, 5, 64)])
def test_backward_at_the_kink_within_bounds(ops, h, w, K, s, lddh, mode):
    """A landmark exactly ON a render pixel whose softmax is NOT saturated (the symmetric pair: mu == 0, and lin_5(2) == 0), so that the term
    sign(0) = 0 removes reaches dheat: mu, py, px are the exact heat-maps' predicted ones, dgauss is dense."""
    e = R.exact_heat(h, w, K)
    mu, py, px = dev(T32(e.mu)), dev(T32(e.py)), dev(T32(e.px))
    dy, dx = R.offsets(e.mu, s)
    open_y = ((dy == 0).any(1) & (e.py.max(1) < 1)) | ((dx == 0).any(1) & (e.px.max(1) < 1))
    assert open_y.any(), 'no unsaturated landmark sits on a pixel'
    worst = {}
    for dt in R.STORAGE:
        dg = R.dense_dg(e.B, s, K, dt)
        r = R.backward(R.widen(dg), e.mu, e.py, e.px, 10.0, mode)
        assert float(np.abs(r.dheat[:, :, :, open_y.any(0)]).max()) > 0
        key = bits(dt)
        dheat = run_bwd(ops, dg, mu, py, px, h, w, 10.0, mode, lddh)
        worst[key] = max(worst.get(key, 0.0), held(dheat[..., :K], r.dheat, r.bound, dt, 'dheat at the kink %s %s' % (mode, dt)))
        if dt != F32:
            o = run_head_bwd(ops, dg, mu, py, px, h, w, 10.0, mode, lddh, R.selector(48, K, lddh), 48)
            same_bits(o.dheat, dheat, 'fused vs standalone dheat at the kink %s' % dt)
    report('backward at the kink %s %dx%dx%d' % (mode, h, w, K), **worst)


def given_mu(B, K, s):
    """Landmarks handed to the render-only kernels: exactly +-1, +-1.5 (edited landmarks leave the square), on a pixel, between pixels."""
    g = np.random.RandomState(B + K + s)
    mu = g.uniform(-1, 1, (B, K, 2)).astype(np.float32)
    lin = R.lin_pm1(s)
    fixed = [(-1, 1), (1, -1), (1.5, -1.5), (-1.5, 0.25), (lin[s // 2], lin[0]), (lin[-1], lin[s // 3]),
             (0.5 * (float(lin[0]) + float(lin[min(1, s - 1)])), 0.0)]
    for i, v in enumerate(fixed[:K]):
        mu[i % B, i % K] = v
    return mu


@MODE
@pytest.mark.parametrize('s,K', [(1, 7), (5, 7), (16, 11), (128, 3)])
def test_render_only_kernels_within_bounds(ops, s, K, mode):
    """B5: imm_softargmax_gauss_fwd's render-only mode in three storage types and imm_gauss_render_f32, from given landmarks."""
    B, worst = 2, {}
    mu = given_mu(B, K, s)
    ref, bound = R.render(mu, s, 10.0, mode)
    mud = dev(T32(mu))
    for dt in R.STORAGE:
        joint = gout((B, s, s, K + 3), dt)
        ops.gauss_render_fwd(mud, B, K, 10.0, s, joint, K + 3, dt, mode)
        torch.cuda.synchronize()
        assert untouched(joint[..., K:])
        worst[bits(dt)] = max(worst.get(bits(dt), 0.0), held(joint[..., :K], ref, bound, dt, 'render-only %s %s' % (mode, dt)))
        if dt == F32:
            out = gout((B, s, s, K), F32)
            ops.gauss_render_f32(mud, B, K, 10.0, s, out, mode)
            torch.cuda.synchronize()
            same_bits(out, joint[..., :K].contiguous(), 'gauss_render_f32 vs the render-only mode')
    report('render-only %s s%d K%d' % (mode, s, K), **worst)


def test_render_f32_grid_stride_loop(ops):
    """B5: more than 8192 * 256 values, so that gauss_render_f32's grid-stride loop takes a second trip."""
    B, K, s = 3, 43, 128
    assert B * s * s * K > 8192 * 256
    mu = given_mu(B, K, s)
    out = gout((B, s, s, K), F32)
    ops.gauss_render_f32(dev(T32(mu)), B, K, 10.0, s, out, 'rot')
    torch.cuda.synchronize()
    ref, bound = R.render(mu, s, 10.0, 'rot')
    report('gauss_render_f32, second trip', maps=held(out, ref, bound, F32, 'gauss_render_f32'))


@MODE
@pytest.mark.parametrize('dt', R.STORAGE, ids=R.STORAGE_IDS)
def test_render_only_equals_the_softargmax_tail(ops, dt, mode):
    """B5: the same mu gives the same bits from the soft-argmax tail, the render-only mode and (f32) imm_gauss_render_f32."""
    B, h, w, K, s = 3, 8, 8, 10, 16
    o = run_fwd(ops, R.bump_heat(B, h, w, K), s, 10.0, mode, dt)
    joint = gout((B, s, s, K + 3), dt)
    ops.gauss_render_fwd(o.mu, B, K, 10.0, s, joint, K + 3, dt, mode)
    torch.cuda.synchronize()
    same_bits(joint[..., :K].contiguous(), o.g.contiguous(), 'render-only vs the tail %s %s' % (mode, dt))
    if dt == F32:
        out = gout((B, s, s, K), F32)
        ops.gauss_render_f32(o.mu, B, K, 10.0, s, out, mode)
        torch.cuda.synchronize()
        same_bits(out, o.g.contiguous(), 'gauss_render_f32 vs the tail')


# ==============================================================================================
# C. limits
# ==============================================================================================
def refused(err, outs, fn, what):
    with pytest.raises(err):
        fn()
    torch.cuda.synchronize()
    for o in outs:
        assert untouched(o), '%s: a refused call wrote an output' % what


@pytest.mark.parametrize('what,C,K,h,w,dt', [('k = 65', 32, 65, 4, 4, BF16), ('c = 48', 48, 3, 4, 4, BF16), ('h w = 24', 32, 3, 4, 6, BF16),
                                              ('LDS over the cap', 32, 40, 32, 32, BF16), ('f32 storage', 32, 3, 4, 4, F32)])
def test_pose_head_forward_refuses(ops, lib_error, what, C, K, h, w, dt):
    B, s, ldh, ldg = 1, 4, K + 3, K + 5
    sdt = BF16 if dt == F32 else dt
    feat, wt = dev(torch.zeros((B, h, w, C), dtype=sdt)), dev(torch.zeros((80, C + 32), dtype=sdt))
    outs = [gout((B, h, w, ldh), F32), gout((B, K, 2), F32), gout((B, h, K), F32), gout((B, w, K), F32), gout((B, s, s, ldg), sdt)]
    refused(lib_error, outs, lambda: ops.pose_head_fwd(feat, C, C, wt, dev(torch.zeros(K)), B, h, w, K, 10.0, s, outs[0], ldh, outs[1], outs[2],
                                                      outs[3], outs[4], ldg, dt, 'rot'), what)


def test_softargmax_forward_refuses_a_heat_map_over_the_lds_cap(ops, lib_error):
    B, h, w, K, s = 1, 32, 32, 40, 4
    assert R.fwd_lds(h, w, K) > R.LDS_CAP
    outs = [gout((B, K, 2), F32), gout((B, h, K), F32), gout((B, w, K), F32), gout((B, s, s, K), BF16)]
    heat = dev(torch.zeros((B, h, w, K)))
    refused(lib_error, outs, lambda: ops.softargmax_gauss_fwd(heat, K, B, h, w, K, 10.0, s, outs[0], outs[1], outs[2], outs[3], K, BF16, 'rot'), 'LDS')


@pytest.mark.parametrize('what,C,lddh,h,w', [('lddh = 48', 32, 48, 4, 4), ('c = 24', 24, 32, 4, 4), ('LDS over the cap', 32, 64, 32, 48)])
def test_pose_head_backward_refuses(ops, lib_error, what, C, lddh, h, w):
    B, K, s = 1, 3, 4
    if what.startswith('LDS'):
        assert R.bwd_lds(h, w, K, lddh) > R.LDS_CAP
    dg, wtd = dev(torch.zeros((B, s, s, K), dtype=BF16)), dev(torch.zeros((32, 64), dtype=BF16))
    mu, py, px = dev(torch.zeros((B, K, 2))), dev(torch.zeros((B, h, K))), dev(torch.zeros((B, w, K)))
    outs = [gout((B, h, w, lddh), BF16), gout((B, h, w, 32), BF16), gout((B, K), F32)]
    refused(lib_error, outs, lambda: ops.pose_head_bwd(dg, K, B, h, w, K, 10.0, s, mu, py, px, outs[0], lddh, wtd, C, outs[1], 32, outs[2], 'rot'), what)


def test_render_only_refuses_a_batch_of_65536(ops, lib_error):
    """Arguments only: the entry point refuses before any launch, so nothing of that size exists."""
    K, s = 3, 4
    out = gout((2, s, s, K), BF16)
    refused(lib_error, [out], lambda: ops.gauss_render_fwd(dev(torch.zeros((2, K, 2))), 65536, K, 10.0, s, out, K, BF16, 'rot'), 'batch = 65536')
