"""The exact-arithmetic kernel tests (tests/test_exact_gpu.py), validated without a GPU: the helper on hand-made values, and every
case and type of the GPU tables on the reference alone —

  exactness      max(sum_k |x||w| + |bias|) < 2^24 for outputs, sum_pixels |x||dy| < 2^24 for filter gradients, and for the
                 batch-norm partial sums 4 x the launch-wide sum v^2 (and sum |v * mask|) of a channel < 2^24 (the factor four
                 covers the half-integer bias): every partial row, in any order, is then exact in f32;
  no saturation  max|ref| <= finfo(dt).max / 2;
  the rounding is exercised: in every 16-bit high-amplitude run >= 20 % of the outputs are not representable in dt, >= 5 % are
                 exact ties and >= 5 % inexact non-ties (a test of the store's rounding on data that never rounds proves nothing);
  the sums tell v from its rounding: in every 16-bit batch-norm-sum run the sums of the ROUNDED stored value, (sum r, sum r^2) and
                 (sum r, sum r * mask) with r = RNE16(v), differ from the exact sums of v in at least one channel (else a kernel that
                 sums what it stored would pass).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as E                                                       # noqa: E402

DT = pytest.mark.parametrize('dt', E.DTYPES, ids=E.DT_IDS)


# ---- the helper ------------------------------------------------------------------------------
def test_rne16_ties_to_even_both_ways_and_a_non_tie():
    bf = torch.bfloat16
    # bf16 keeps 8 significant bits: between 256 and 512 the representable values are the even integers
    v = torch.tensor([259.0, 257.0, 258.5, -259.0, -257.0, 300.0, 0.5], dtype=torch.float64)
    want = torch.tensor([260.0, 256.0, 258.0, -260.0, -256.0, 300.0, 0.5], dtype=torch.float32)
    #                    tie up  tie down non-tie
    assert torch.equal(E.rne16(v, bf).view(bf).float(), want)
    # f16 keeps 11: between 2048 and 4096 likewise
    v = torch.tensor([2051.0, 2049.0, 2050.5, 4100.0], dtype=torch.float64)
    want = torch.tensor([2052.0, 2048.0, 2050.0, 4100.0], dtype=torch.float32)
    assert torch.equal(E.rne16(v, torch.float16).view(torch.float16).float(), want)


def test_rne16_rejects_what_is_not_exact_in_f32_and_what_saturates():
    with pytest.raises(AssertionError, match='not exact in f32'):
        E.rne16(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64), torch.bfloat16)
    with pytest.raises(AssertionError, match='saturates'):
        E.rne16(torch.tensor([70000.0], dtype=torch.float64), torch.float16)
    with pytest.raises(AssertionError, match='REFERENCE'):
        E.rne16(torch.tensor([float('nan')], dtype=torch.float64), torch.bfloat16)


def test_roundings_and_mix():
    v = torch.tensor([259.0, 257.0, 258.5, 258.0, -259.0, -261.5], dtype=torch.float64)
    rne, trunc, away, inexact, tie = E.roundings(v, torch.bfloat16)
    as_f = lambda b: b.view(torch.bfloat16).float().tolist()                 # noqa: E731
    assert as_f(rne) == [260.0, 256.0, 258.0, 258.0, -260.0, -262.0]
    assert as_f(trunc) == [258.0, 256.0, 258.0, 258.0, -258.0, -260.0]
    assert as_f(away) == [260.0, 258.0, 258.0, 258.0, -260.0, -262.0]
    assert inexact.tolist() == [True, True, True, False, True, True] and tie.tolist() == [True, True, False, False, True, False]
    assert E.rounding_mix(v, torch.bfloat16) == (5 / 6, 3 / 6, 2 / 6)


@DT
def test_exact_equal_passes_on_the_rne_bits_and_on_exact_f32(dt):
    v = torch.tensor([[259.0, 257.0, 258.5, -0.5, 0.0, 1000.0]], dtype=torch.float64)
    E.exact_equal(v.float().to(dt), E.rne16(v, dt), 'rne', exact=v)
    E.exact_equal(v.float(), v, 'f32')
    E.exact_equal(v.clone(), v, 'f64')


def test_exact_equal_names_truncation_and_ties_away():
    bf = torch.bfloat16
    v = torch.tensor([300.0, 259.0, 257.0, 258.5, 261.5], dtype=torch.float64)
    want = E.rne16(v, bf)
    trunc = torch.tensor([300.0, 258.0, 256.0, 258.0, 260.0]).to(bf)
    with pytest.raises(AssertionError, match=r'2/5 elements differ.*first at \(1,\) got 258.0 want 260.0.*TRUNCATED.*2 match truncation'):
        E.exact_equal(trunc, want, 'trunc', exact=v)
    away = torch.tensor([300.0, 260.0, 258.0, 258.0, 262.0]).to(bf)
    with pytest.raises(AssertionError, match=r'1/5 elements differ.*first at \(2,\) got 258.0 want 256.0.*TIES-AWAY'):
        E.exact_equal(away, want, 'away', exact=v)
    twice = torch.tensor([300.0, 260.0, 256.0, 260.0, 262.0]).to(bf)          # 258.5 -> 259 (a coarser hop) -> 260: neither
    with pytest.raises(AssertionError, match='neither'):
        E.exact_equal(twice, want, 'twice', exact=v)


def test_exact_equal_fails_on_nan_inf_and_one_ulp_and_blames_a_bad_reference():
    v = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    for bad in (float('nan'), float('inf'), 2.0 + 2.0 ** -22):
        got = v.float().clone()
        got[1] = bad
        with pytest.raises(AssertionError, match='1/3 elements differ'):
            E.exact_equal(got, v, 'f32')
    got = v.float().to(torch.bfloat16)
    got[2] = float('nan')
    with pytest.raises(AssertionError, match=r'1/3 elements differ \(1 NaN'):
        E.exact_equal(got, E.rne16(v, torch.bfloat16), 'nan16')
    with pytest.raises(AssertionError, match='REFERENCE'):
        E.exact_equal(v.float(), torch.tensor([1.0, float('nan'), 3.0], dtype=torch.float64), 'badref')
    with pytest.raises(AssertionError, match='REFERENCE'):
        E.exact_equal(torch.full((3,), float('nan')), torch.tensor([1.0, float('nan'), 3.0], dtype=torch.float64), 'badref')
    # -0 and +0 are different bits: a masked or clamped output is +0
    with pytest.raises(AssertionError, match='1/1 elements differ'):
        E.exact_equal(torch.tensor([-0.0]), torch.tensor([0.0], dtype=torch.float64), 'zero')


# ---- the tables ------------------------------------------------------------------------------
def _is_16bit_exercised(v, dt, what):
    n_inexact, n_tie, n_other = E.rounding_mix(v, dt)
    assert n_inexact >= 0.20 and n_tie >= 0.05 and n_other >= 0.05, \
        '%s: %.1f %% not representable, %.1f %% ties, %.1f %% inexact non-ties (need 20 / 5 / 5)' % (
            what, 100 * n_inexact, 100 * n_tie, 100 * n_other)


def _fits(v, bound, dt, what):
    assert float(bound.max()) < E.LIMIT, '%s: sum of |terms| reaches %.3g >= 2^24' % (what, float(bound.max()))
    assert float(v.abs().max()) <= 0.5 * torch.finfo(dt).max, '%s: max|ref| %.6g saturates %s' % (what, float(v.abs().max()), dt)
    assert bool((v.abs() <= bound).all())


def _stats_fit(v, mask, what):
    s2 = 4 * float((v * v).sum((0, 1, 2)).max())
    sm = 4 * float((torch.where(mask > 0, v, 0.) * mask).abs().sum((0, 1, 2)).max())
    assert s2 < E.LIMIT and sm < E.LIMIT, '%s: 4 x sum v^2 = %.3g, 4 x sum |v mask| = %.3g (limit 2^24 = %.3g)' % (what, s2, sm, E.LIMIT)


def _sums_tell_v_from_its_rounding(v, mask, dt, what):
    """A kernel that summed r = RNE16(v), the value it stored, instead of the f32 v must miss the exact sums of this run."""
    def differ(v, second):
        r = v.float().to(dt).to(E.F64)
        s = lambda t: t.sum((0, 1, 2))                                        # noqa: E731
        return int(((s(r) != s(v)) | (s(second(r)) != s(second(v)))).sum())
    n = differ(v, lambda t: t * t)
    assert n > 0, '%s: (sum r, sum r^2) of the rounded outputs equal the exact sums in every channel' % what
    if mask is not None:
        n = differ(torch.where(mask > 0, v, 0.), lambda t: t * mask)
        assert n > 0, '%s: (sum r, sum r * mask) of the rounded outputs equal the exact sums in every channel' % what


@DT
@pytest.mark.parametrize('tag', E.FWD_TAGS)
def test_forward_case_meets_the_conditions(tag, dt):
    out_f32 = E.fwd_shapes()[tag][7]
    e = E.fwd_data(tag, dt, low=False, bounds=True)
    _fits(e.y, e.y_bound, dt, tag)
    if not out_f32:
        _is_16bit_exercised(e.y, dt, tag + '/bias')
        _is_16bit_exercised(e.y.clamp(min=0), dt, tag + '/relu')
        _is_16bit_exercised(torch.where(e.mask > 0, e.y, 0.), dt, tag + '/mask')
    assert bool((e.mask > 0).any()) and bool((e.mask < 0).any()) and bool((e.mask == 0).any())
    lo = E.fwd_data(tag, dt, low=True, bounds=True)
    _fits(lo.y, lo.y_bound, dt, tag + '/low')
    _stats_fit(lo.y, lo.mask, tag + '/low')
    if not out_f32:                                        # (an f32 output is not rounded: there the sums and the store both hold v)
        _sums_tell_v_from_its_rounding(lo.y, lo.mask, dt, tag + '/low')


@DT
@pytest.mark.parametrize('B,S,co', E.FIRST_CASES)
def test_first_conv_case_meets_the_conditions(B, S, co, dt):
    e = E.first_data(B, S, co, dt, low=False, bounds=True)
    _fits(e.y, e.y_bound, dt, 'conv_first')
    _is_16bit_exercised(e.y, dt, 'conv_first/bias')
    _is_16bit_exercised(e.y.clamp(min=0), dt, 'conv_first/relu')
    lo = E.first_data(B, S, co, dt, low=True, bounds=True)
    _fits(lo.y, lo.y_bound, dt, 'conv_first/low')
    s2 = 4 * float((lo.y * lo.y).sum((0, 1, 2)).max())
    assert s2 < E.LIMIT, s2
    _sums_tell_v_from_its_rounding(lo.y, None, dt, 'conv_first/low')


def _dgrad_cases():
    out = [('dgrad', tag, (s[0], s[1], s[2], s[4], s[6], s[7]), amps) for tag, (s, _key, amps) in E.DGRAD.items()]
    (B, H, ci, co), _key, amps = E.GROUP
    out.append(('group', 'group', (B, H, ci, co, 3, 2), amps))
    out += [('s2d', tag, (B, H, ci, co, 3, 2), amps) for tag, ((B, H, ci, co), amps) in E.S2D.items()]
    out += [('tap', tag, (B, H, ci, co, 3, 1), amps) for tag, ((B, H, ci, co, _l1), amps) in E.TAP.items()]
    return out


@DT
@pytest.mark.parametrize('kind,tag,shape,amps', _dgrad_cases(), ids=['%s_%s' % c[:2] for c in _dgrad_cases()])
def test_data_gradient_case_meets_the_conditions(kind, tag, shape, amps, dt):
    e = E.dgrad_data(kind, tag, shape, dt, amps, bounds=True)
    # (the tap adds at most |coef mask (a_pred - a_gt)| <= 12 to a rounded value: far inside both limits)
    _fits(e.dx, e.dx_bound + (12 if kind == 'tap' else 0), dt, tag)
    _is_16bit_exercised(e.dx, dt, '%s/%s' % (kind, tag))


@DT
@pytest.mark.parametrize('tag', list(E.WGRAD))
def test_filter_gradient_case_is_exact(tag, dt):
    B, H, ci_real, _ci_pad, co, _lddy, k, kw, stride, _nsplit, _key = E.WGRAD[tag]
    e = E.wgrad_data(tag, B, H, ci_real, co, k, kw, stride, dt, 5, bounds=True)
    assert float(e.dw_bound.max()) < E.LIMIT and float(e.dw.abs().max()) > 0


@DT
def test_filter_gradient_multi_jobs_are_exact(dt):
    for i, (B, H, ci, co, _lddy, k, stride, _ns) in enumerate(E.WGRAD_MULTI):
        e = E.wgrad_data('multi%d' % i, B, H, ci, co, k, k, stride, dt, 500 + i, bounds=True)
        assert float(e.dw_bound.max()) < E.LIMIT and float(e.dw.abs().max()) > 0, i


@DT
def test_plain_sums_are_exact(dt):
    a, b, mask = E.sse_data(dt)
    d = a - b
    m4 = mask[:, ::2, ::2].unsqueeze(-1)
    assert float((m4 * d * d).sum()) < E.LIMIT and float((m4 * d.abs()).sum()) < E.LIMIT
    x = E.colsum_data(dt)
    assert float(x.abs().sum(0).max()) < E.LIMIT
