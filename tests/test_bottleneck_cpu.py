"""tests/bottleneck_reference.py and the data of tests/test_bottleneck_gpu.py, pinned without a GPU.

  the reference   agrees with oracle/imm_oracle.py (soft_argmax, gaussian_maps) and with torch.autograd in f64 to 1e-9 when it is given
                  the oracle's f64 linspace in place of the kernel's f32 lin_pm1 (which is within one f32 rounding of it); at the kink
                  every mode's gradient term is exactly 0.
  exact data      every exact heat-map meets its premises: integers representable in f32, the winners' means equal bit for bit in the
                  f32 emulation, every other exponent below -104, the predicted mu, py, px equal to the emulation's; and the sets hold
                  what they are there for (first and last row, mu == 0, an off-grid mu, a landmark on a render pixel).
  bounded data    nothing is left out of a bounded comparison (asserted: share 0, cap 1 %), the bump family reaches the edges
                  (max |mu| > 0.9), its 'rot' maps hold values above the old absolute tolerance, the 16-bit outputs round, and the
                  bounds are finite, positive and grow with K, h and s as the counting says.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import imm_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bottleneck_reference as R                                             # noqa: E402

T64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731
EXACT_MAPS = [(16, 16), (5, 12), (32, 16), (1, 7), (4, 4)]
EXACT_K = [1, 7, 11, 64]
LEFT_OUT_CAP = 0.01


@pytest.fixture(scope='module', autouse=True)
def _release_cases():
    yield
    R.clear_cache()


@pytest.fixture
def oracle_lin(monkeypatch):
    """The reference on the oracle's f64 linspace: what is compared is the rule, not the last place of lin."""
    monkeypatch.setattr(R, 'lin_pm1', lambda n: O.linspace_pm1(n, torch.float64).numpy())


def rel_close(got, ref, tol, what, keep=None):
    got, ref = np.asarray(got), np.asarray(ref)
    err = np.abs(got - ref) / (np.abs(ref).max() + 1e-300)
    if keep is not None:
        err = err[keep]
    assert float(err.max()) <= tol, '%s: %.3g' % (what, float(err.max()))


# ---- the reference against the oracle and autograd --------------------------------------------
def test_lin_pm1_is_within_one_rounding_of_the_oracle_linspace():
    differs = []
    for n in range(1, 130):
        a, b = R.lin_pm1(n).astype(np.float64), O.linspace_pm1(n, torch.float64).numpy()
        assert a.shape == b.shape and float(np.abs(a - b).max()) <= 2.0 ** -24, n        # one f32 rounding of a value below 1
        if not np.array_equal(a.astype(np.float32), b.astype(np.float32)):
            differs.append(n)
    assert R.lin_pm1(1)[0] == -1 and 12 in differs, differs


@pytest.mark.parametrize('K', [1, 7, 11, 64])
@pytest.mark.parametrize('h,w,s', [(8, 8, 16), (5, 12, 7), (16, 8, 5)])
def test_forward_equals_the_oracle(oracle_lin, h, w, s, K):
    heat = R.bump_heat(2, h, w, K).astype(np.float64)
    f = R.forward(heat)
    mu, py, px = O.soft_argmax(T64(heat))
    rel_close(f.mu, mu.numpy(), 1e-12, 'mu'); rel_close(f.py, py.numpy(), 1e-12, 'py'); rel_close(f.px, px.numpy(), 1e-12, 'px')
    for mode in R.MODES:
        g, b = R.render(f.mu, s, 10.0, mode)
        rel_close(g, O.gaussian_maps(mu, [s, s], 10.0, mode).numpy(), 1e-9, 'maps ' + mode)
        assert np.isfinite(b).all() and (b > 0).all()


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('h,w,s,K', [(8, 8, 16, 7), (5, 12, 7, 11), (16, 8, 5, 1), (4, 4, 6, 64)])
def test_backward_equals_autograd(oracle_lin, h, w, s, K, mode):
    heat = R.randn_heat(2, h, w, K, 2.0).astype(np.float64)
    dg = R.widen(R.dense_dg(2, s, K, torch.float32))
    hr = T64(heat).requires_grad_(True)
    mu, py, px = O.soft_argmax(hr)
    (gh,) = torch.autograd.grad(O.gaussian_maps(mu, [s, s], 10.0, mode), hr, T64(dg))
    r = R.backward(dg, mu.detach().numpy(), py.detach().numpy(), px.detach().numpy(), 10.0, mode)
    dy, dx = R.offsets(mu.detach().numpy(), s)
    assert min(float(np.abs(dy).min()), float(np.abs(dx).min())) > 1e-6, 'a pixel on the kink: autograd is no reference there'
    rel_close(r.dheat, gh.numpy(), 1e-9, 'dheat ' + mode)
    assert np.isfinite(r.bound).all() and (r.bound > 0).all()


@pytest.mark.parametrize('mode', R.MODES)
def test_the_gradient_term_at_the_kink_is_exactly_zero(mode):
    z = np.zeros((1,))
    g, gy, gx = R.gauss_grad(z, z, 10.0, mode)
    assert gy[0] == 0 and gx[0] == 0 and np.isfinite(g[0])
    v, b = R.on_landmark(10.0, mode)
    want = {'rot': 1.0, 'flat': np.exp(-R.C5 ** 0.25), 'ankush': np.exp(-np.sqrt(R.C4)) ** 2}[mode]
    assert abs(v - want) <= 1e-15 and 0 < b < 1e-6
    # one axis on the landmark, the other not: only that axis' term vanishes
    _g, gy, gx = R.gauss_grad(z, z + 0.25, 10.0, mode)
    assert gy[0] == 0 and gx[0] != 0


# ---- exact data -------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [0, R.SHIFT])
@pytest.mark.parametrize('K', EXACT_K)
@pytest.mark.parametrize('h,w', EXACT_MAPS)
def test_exact_heat_maps_meet_their_premises(h, w, K, shift):
    e = R.exact_heat(h, w, K)
    heat = e.heat + shift
    assert R.exact_in_f32(heat) and float(heat.max()) * max(h, w) < 2 ** 24          # every partial sum of a mean is an integer below 2^24
    rm, cm = R.means_f32(heat)
    for b, k, Y, X in e.sets:
        assert len(set(rm[b, Y, k].tolist())) == 1 and len(set(cm[b, X, k].tolist())) == 1, 'the winners must tie bit for bit'
        assert len(Y) in (1, 2, 4) and len(X) in (1, 2, 4)
    mu, py, px, worst = R.softargmax_f32(heat)
    assert np.isfinite(mu).all() and worst < -104, worst
    assert np.array_equal(mu, e.mu) and np.array_equal(py, e.py) and np.array_equal(px, e.px)
    assert set(np.unique(py).tolist()) <= {0.0, 0.25, 0.5, 1.0}
    # the f64 rule agrees: the premises make the f32 result the exact one up to the roundings of mu
    f = R.forward(heat)
    assert float(np.abs(f.mu - mu).max()) <= 4 * R.U and float(np.abs(f.py - py).max()) < 1e-40


def test_exact_sets_hold_the_edges_they_are_for():
    e = R.exact_heat(16, 16, 11)
    lin = R.lin_pm1(16)
    Ys = [tuple(Y) for _b, _k, Y, _X in e.sets]
    assert (0,) in Ys and (15,) in Ys and (0, 15) in Ys and (0, 1) in Ys
    assert (e.mu[..., 0] == -1).any() and (e.mu[..., 0] == 1).any() and (e.mu[..., 1] == -1).any() and (e.mu[..., 1] == 1).any()
    assert (e.mu == 0).any(), 'the symmetric pair'
    off = ~np.isin(e.mu, lin)
    assert off.any(), 'the asymmetric pair gives an off-grid mu'
    on = np.isin(e.mu[..., 0], lin) & np.isin(e.mu[..., 1], lin)
    assert on.any(), 'with s == h a landmark sits exactly on a render pixel'
    dy, dx = R.offsets(e.mu, 16)
    assert ((dy == 0).any(1) & (dx == 0).any(1)).any()
    for h, w in EXACT_MAPS:
        assert len(R.index_sets(h)) >= 2 and all(max(i) < h for i in R.index_sets(h)) and all(max(i) < w for i in R.index_sets(w))
    o = R.one_hot_heat(8, 8, 11)
    assert ((o.py == 1).sum(1) == 1).all() and ((o.px == 1).sum(1) == 1).all() and (o.mu[:, 0] == [-1, 1]).all()
    mu, py, px, worst = R.softargmax_f32(o.heat)
    assert np.array_equal(mu, o.mu) and np.array_equal(py, o.py) and np.array_equal(px, o.px) and worst < -104


# ---- bounded data -----------------------------------------------------------------------------
def test_the_bump_family_reaches_the_edges_and_fills_the_maps():
    for B, h, w, K in [(3, 8, 8, 10), (3, 16, 8, 33), (2, 16, 16, 64), (3, 5, 12, 21)]:
        f = R.forward(R.bump_heat(B, h, w, K).astype(np.float64))
        assert float(np.abs(f.mu).max()) > 0.9, (h, w, K, float(np.abs(f.mu).max()))
        # exp(-100 r^2) > 1e-3 inside r < 0.263: 5.4 % of the square at most, wherever the landmarks lie.  The bounded cases
        # therefore render at inv_std 3 as well (R.INV_STDS), where the disc has r < 0.876
        g, _b = R.render(f.mu.astype(np.float32), 16, R.INV_STDS[1], 'rot')
        share = (g > 1e-3).mean((1, 2, 3))
        assert float(share.max()) >= 0.30, (h, w, K, share)
        g, _b = R.render(f.mu.astype(np.float32), 16, R.INV_STDS[0], 'rot')
        assert float((g > 1e-3).mean()) < 0.06
    old = R.forward(R.randn_heat(3, 16, 16, 10, 2.0).astype(np.float64))
    assert float(np.abs(old.mu).max()) < 0.5, 'the family the earlier tests use stays in the centre'
    sat = R.forward(R.randn_heat(3, 8, 8, 10, 30.0).astype(np.float64))
    assert float(sat.py.max()) > 0.99, 'randn * 30 is near-saturated'


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('h,w,s,K', [(8, 8, 16, 11), (5, 12, 5, 21), (16, 8, 16, 64)])
def test_nothing_is_left_out_and_the_outputs_round(h, w, s, K, mode):
    f = R.forward_bounds(R.bump_heat(3, h, w, K).astype(np.float64))
    mu32, py32, px32 = f.mu.astype(np.float32), f.py.astype(np.float32), f.px.astype(np.float32)
    g, gb = R.render(mu32, s, 10.0, mode)
    tables = [f.e_mu, f.e_py, f.e_px, gb]
    for dt in (R.BF16, R.F16):
        dg = R.widen(R.dense_dg(3, s, K, dt))
        r = R.backward(dg, mu32, py32, px32, 10.0, mode)
        tables.append(r.bound)
        left_out = ~np.isfinite(r.bound) | ~np.isfinite(r.dheat)
        assert float(left_out.mean()) == 0.0 <= LEFT_OUT_CAP                  # found: 0 in every case; nothing needs leaving out
        assert R.rounds_in(r.dheat, dt) > 0.5 and R.rounds_in(g, dt) > 0.5
        assert float(np.abs(r.dheat).max()) > 0
        # the bound counts roundings: before the 16-bit store it is everywhere below a hundredth of the 1e-2 |ref| + 2e-3 max that
        # the oracle parity test allows
        old = 1e-2 * np.abs(r.dheat) + 2e-3 * np.abs(r.dheat).max()
        assert float((r.bound / old).max()) < 1e-2, float((r.bound / old).max())
    for t in tables:
        assert np.isfinite(t).all() and (t > 0).all()


def test_the_bounds_grow_as_the_counting_says():
    assert R.depth(5, 256) == 1 + 6 + 4 and R.depth(16, 256) == 11 and R.depth(24, 256) == 13 and R.depth(16, 512) == 1 + 6 + 8
    assert R.depth(128, 256) > R.depth(24, 256) > R.depth(16, 256)
    heat = R.randn_heat(2, 8, 8, 4, 2.0).astype(np.float64)
    wide = np.concatenate([heat, heat], 2)                                  # twice the columns, the same means
    a, b = R.forward_bounds(heat), R.forward_bounds(wide)
    assert (b.e_py > a.e_py).all() and (b.e_mu[..., 0] > a.e_mu[..., 0]).all()
    f = R.forward(heat)
    mu32, py32, px32 = f.mu.astype(np.float32), f.py.astype(np.float32), f.px.astype(np.float32)
    dg = R.widen(R.dense_dg(2, 16, 4, R.BF16))
    one, deep = R.backward(dg, mu32, py32, px32, 10.0, 'rot', single=True), R.backward(dg, mu32, py32, px32, 10.0, 'rot', nthr=512)
    mid = R.backward(dg, mu32, py32, px32, 10.0, 'rot')
    assert (one.bound < mid.bound).all() and (mid.bound < deep.bound).all()
    d16 = R.widen(R.store(np.random.RandomState(1).standard_normal((2, 4, 4, 64)), R.BF16))
    wt = R.selector(32, 64, 64) + R.selector(32, 33, 64, 1)
    _r, b8, _s, sb8 = R.head_dgrad(d16, wt, 8)
    _r, b64, _s, sb64 = R.head_dgrad(d16, wt, 64)
    assert (b64 >= b8).all() and (b64 > b8).any() and np.isfinite(b64).all() and (sb8 > 0).all() and (sb64 > 0).all()
    assert R.fwd_lds(16, 16, 64) > R.LDS_OPT_IN and R.fwd_lds(32, 32, 40) > R.LDS_CAP > R.fwd_lds(16, 16, 64)
    assert R.LDS_CAP > R.bwd_lds(32, 16, 3, 64) > R.LDS_OPT_IN and R.bwd_lds(32, 48, 3, 64) > R.LDS_CAP


def test_the_window_rule():
    ref = np.array([1.0, 1.0, 1.0, 1.0, 0.0, 3e-6])
    for dt, ulp in ((R.BF16, 2.0 ** -7), (R.F16, 2.0 ** -10)):
        # a bound of 3/4 ulp lets the neighbour in, one of 1/4 ulp (and the tie at 1/2, which RNE sends back to 1.0) does not
        bound = np.array([0.0, 0.0, 0.75 * ulp, 0.5 * ulp, 0.0, 0.0])
        got = np.array([1.0, 1.0 + ulp, 1.0 + ulp, 1.0 + ulp, -0.0, float(R.widen(R.store(np.array([3e-6]), dt))[0])])
        assert R.window(got, ref, bound, dt).tolist() == [False, True, False, True, False, False]
        assert R.window(np.array([np.nan]), ref[:1], bound[:1], dt).all()
    assert R.window(np.array([1.0 + 2e-7, np.nan]), np.ones(2), np.full(2, 1e-7), torch.float32).all()
    assert not R.window(np.array([1.0 + 5e-8]), np.ones(1), np.full(1, 1e-7), torch.float32).any()


def test_single_pixel_gradients_hold_one_value_per_landmark():
    for dt in R.STORAGE:
        dg = R.widen(R.single_dg(3, 5, 11, dt))
        assert ((dg != 0).sum((1, 2)) == 1).all() and float(np.abs(dg[dg != 0]).min()) > 0.1
    s = R.selector(144, 3, 32)
    assert ((s != 0).sum(1) == 1).all() and (s[:, 3:] == 0).all() and set(np.abs(s[s != 0]).tolist()) <= {1.0, 2.0, 4.0}
