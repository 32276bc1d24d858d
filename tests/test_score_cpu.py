"""Landmark quality without a GPU: the numpy restatement of include/imm_score.h (tests/score_reference.py) against answers derived
by hand, its NaN and threshold rules, the gated landmarks as bits, and the host side of imm_amd/quality.py (QualityGate, plan_track's
gate argument, Track's new fields)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_reference as SR                      # noqa: E402

F32, F64 = np.float32, np.float64
S = 128


def one_hot(F, n, K, bins):
    q = np.zeros((F, n, K), dtype=F32)
    for f in range(F):
        for k in range(K):
            q[f, bins[f][k], k] = 1.0
    return q


def lin(i, n):
    return F64(-1.0) + (F64(2.0) * F64(i)) / F64(n - 1)


softmax_case = SR.softmax_case


# ----------------------------------------------------------------------------------------------------------------------------
# known answers
# ----------------------------------------------------------------------------------------------------------------------------
def test_one_hot_marginals_at_mu_have_spread_exactly_zero():
    """Grids of 2^m + 1 bins: every bin's coordinate -1 + 2 i / 2^m is an f32, so mu can sit on it exactly and d cancels to 0."""
    F, K, h, w = 2, 5, 17, 9
    rng = np.random.RandomState(0)
    by, bx = rng.randint(0, h, (F, K)), rng.randint(0, w, (F, K))
    py, px = one_hot(F, h, K, by), one_hot(F, w, K, bx)
    coords = np.array([[[lin(by[f, k], h), lin(bx[f, k], w)] for k in range(K)] for f in range(F)])
    mu = coords.astype(F32)
    assert np.array_equal(mu.astype(F64), coords), 'the coordinates are f32 values'
    spread, score, qflags, mu_out, sbar, residual = SR.landmark_scores(py, px, mu, None, None, S)
    assert (spread == 0).all() and (sbar == 0).all() and (residual == 0).all() and (qflags == 0).all() and (score == 0).all()
    # and off the bin by one bin: exactly one bin's width on that axis
    mu2 = mu.copy()
    mu2[0, 0, 0] = F32(lin((by[0, 0] + 1) % h if by[0, 0] + 1 < h else by[0, 0] - 1, h))
    assert SR.landmark_scores(py, px, mu2, None, None, S)[0][0, 0] == F32(2.0 / (h - 1))


@pytest.mark.parametrize('n', [2, 3, 16, 64])
def test_uniform_marginals_about_zero(n):
    """sum_i (1 / n) lin(i)^2 = (n + 1) / (3 (n - 1)) per axis (sum of squares of the symmetric grid), so spread = sqrt(2 (n + 1) / (3 (n - 1)))."""
    K = 4
    q = np.full((1, n, K), 1.0 / n, dtype=F32)
    mu = np.zeros((1, K, 2), dtype=F32)
    spread, score, qflags, _mu, sbar, _r = SR.landmark_scores(q, q, mu, None, None, S)
    # (float)(1 / n) is not 1 / n: the sum carries its relative error of at most 2^-24 (half of that in the root), beside the few ulp of
    # f64 the n additions cost
    want = np.sqrt(2.0 * (n + 1) / (3.0 * (n - 1))) * np.sqrt(F64(F32(1.0 / n)) * n)
    assert abs(sbar[0] - want) <= 8 * np.spacing(want), (sbar[0], want)
    assert spread[0, 0] == F32(sbar[0]) and score[0, 0] == F32(sbar[0])
    if n in (2, 16, 64):                                           # 1 / n is an f32 there: the closed form itself, to a few ulp of f64
        exact = np.sqrt(2.0 * (n + 1) / (3.0 * (n - 1)))
        assert abs(sbar[0] - exact) <= 8 * np.spacing(exact)


def shape_case(K=10, seed=3):
    rng = np.random.RandomState(seed)
    ref = rng.uniform(-0.7, 0.7, (K, 2))
    py, px, _ = softmax_case(1, K, 16, 16, seed)
    return ref, py, px


def residual_of(p, ref, py, px, boxes=None):
    return SR.landmark_scores(py, px, np.asarray(p, dtype=F32)[None], boxes, ref, S)[5][0]


def test_a_similar_copy_of_the_reference_has_no_residual():
    """p an exact rotated, scaled, shifted copy of ref: r2 = 1 - |sum u conj v|^2 / (sum |u|^2 sum |v|^2) cancels to rounding, a few
    2^-53, and the residual to its root, about 1e-8.  The reference is on multiples of 1/64 so that the copy (a quarter turn, a half, a
    shift) holds exactly in f32, the type of mu."""
    ref, py, px = shape_case()
    ref = np.round(ref * 64) / 64
    p = np.stack([-ref[:, 1], ref[:, 0]], axis=1) * 0.5 + 0.25
    assert np.array_equal(p.astype(F32).astype(F64), p)
    r = residual_of(p, ref, py, px)
    assert r < 1e-7, r
    assert residual_of(ref, ref, py, px) < 1e-7


def test_two_points_one_moved_at_right_angles():
    """Two points: ref = (0, 0), (0, 2a) and p = (0, 0), (e, 2a), the second moved by e at right angles to the segment.  As complex
    numbers about their means, u = (-+ a i) and v = -+ (e / 2 + a i): v = c u with c = 1 - (e / 2a) i for BOTH points, so two points fit
    a similarity exactly whatever e is.  Closed form: |sum u conj v|^2 = |c|^2 (sum |u|^2)^2 = den * pv, r2 = 0, residual 0 (to
    rounding).

    The smallest shape that can misfit has three points.  Add (0, a), the midpoint, left where it is: (y, x) rows
        ref  (0, 0), (0, 2a), (0, a)      mean (0, a)       u = (0, -a), (0, a), (0, 0)
        p    (0, 0), (e, 2a), (0, a)      mean (e/3, a)     v = (-e/3, -a), (2e/3, a), (-e/3, 0)
        den = 2 a^2        pv = (e^2/9 + a^2) + (4e^2/9 + a^2) + e^2/9 = 2 a^2 + 2 e^2 / 3
        ar = sum u0 v0 + u1 v1 = a^2 + a^2 = 2 a^2
        ai = sum u0 v1 - u1 v0 = -(-a)(-e/3) - (a)(2e/3) = -a e
        r2 = 1 - (4 a^4 + a^2 e^2) / (2 a^2 (2 a^2 + 2 e^2 / 3)) = (a^2 e^2 / 3) / (4 a^4 + 4 a^2 e^2 / 3) = e^2 / (12 a^2 + 4 e^2)
    With a = 1/4, e = 1/8: r2 = (1/64) / (13/16) = 1/52, residual = 0.138675..."""
    a, e = 0.25, 0.125
    py, px, _ = softmax_case(1, 3, 16, 16, 1)
    ref2, p2 = np.array([[0, 0], [0, 2 * a]]), np.array([[0, 0], [e, 2 * a]])
    assert residual_of(p2, ref2, py[:, :, :2], px[:, :, :2]) < 1e-7
    ref3, p3 = np.array([[0, 0], [0, 2 * a], [0, a]]), np.array([[0, 0], [e, 2 * a], [0, a]])
    want = np.sqrt(e * e / (12 * a * a + 4 * e * e))
    assert abs(want - np.sqrt(1.0 / 52.0)) < 1e-15
    got = residual_of(p3, ref3, py, px)
    assert abs(got - want) <= 1e-12, (got, want)


def test_the_residual_is_unchanged_by_a_further_similarity():
    ref, py, px = shape_case()
    rng = np.random.RandomState(5)
    p = np.round((ref + rng.standard_normal(ref.shape) * 0.05) * 1024) / 1024          # f32 values with bits to spare
    r0 = residual_of(p, ref, py, px)
    assert 0.01 < r0 < 0.5
    q = np.stack([-p[:, 1], p[:, 0]], axis=1) * 0.5 + 0.125        # exact in f32: a quarter turn, a half, a shift
    assert abs(residual_of(q, ref, py, px) - r0) <= 1e-12
    # and through a box: source pixels are a scaled, shifted copy (the same scale on both axes for a square box)
    box = np.array([[0, -20, 30, 236, 286]], dtype=np.int32)
    assert abs(residual_of(p, ref, py, px, box) - r0) <= 1e-12
    # the points of a box are step 1 of imm_track.h: origin + (mu + 1) / 2 * S * (side / S)
    spread, score, qf, mo, sbar, rs = SR.landmark_scores(py, px, p.astype(F32)[None], box, None, S)
    assert rs[0] == 0.0 and score[0, 1] == 0.0


# ----------------------------------------------------------------------------------------------------------------------------
# NaN, thresholds, the gated landmarks
# ----------------------------------------------------------------------------------------------------------------------------
def special_case(F=6, K=10, h=16, w=16, seed=11):
    """F >= 6 faces with a shared reference: face 1 has a NaN marginal, face 2 a NaN landmark; ref_coincident is a reference whose points
    coincide (den == 0)."""
    py, px, mu = softmax_case(F, K, h, w, seed)
    rng = np.random.RandomState(seed + 1)
    ref = rng.uniform(-0.7, 0.7, (K, 2))
    py[1, h // 2, K // 2] = np.nan
    mu[2, K - 1, 1] = np.nan
    return py, px, mu, ref


def test_nan_sets_its_bit_and_equality_passes():
    py, px, mu, ref = special_case()
    spread, score, qflags, mu_out, sbar, residual = SR.landmark_scores(py, px, mu, None, ref, S)
    assert np.isnan(sbar[1]) and np.isnan(sbar[2]) and np.isfinite(sbar[[0, 3, 4, 5]]).all()
    assert qflags[1] & 1 and qflags[2] & 1, 'a NaN marginal or landmark sets bit 0'
    assert qflags[2] & 2, 'a NaN landmark is a NaN point: the residual is NaN as well'
    assert not qflags[1] & 2 and (qflags[[0, 3, 4, 5]] == 0).all(), 'no threshold, finite input: no bit'
    assert np.isnan(spread[1, 5]) and np.isfinite(np.delete(spread[1], 5)).all(), 'the NaN stays with its landmark'
    # coincident reference points: den == 0
    flat = np.tile([[0.25, -0.5]], (len(ref), 1))                  # binary fractions: their mean is exact, every u is 0
    r = SR.landmark_scores(py, px, mu, None, flat, S)
    assert np.isnan(r[5]).all() and (r[2] & 2).all()
    # thresholds equal to a score pass it; the next f64 below fails it
    fin = [0, 3, 4, 5]
    ts, tr = sbar[3], residual[4]
    q = SR.landmark_scores(py, px, mu, None, ref, S, ts, tr)[2]
    assert not q[3] & 1 and not q[4] & 2
    assert [bool(q[f] & 1) for f in fin] == [bool(sbar[f] > ts) for f in fin] and [bool(q[f] & 2) for f in fin] == [bool(residual[f] > tr) for f in fin]
    q = SR.landmark_scores(py, px, mu, None, ref, S, np.nextafter(ts, 0), np.nextafter(tr, 0))[2]
    assert q[3] & 1 and q[4] & 2
    # the flags are decided in f64, not on the stored f32: a face whose f32 score lies BELOW its f64 score fails a threshold at the f32
    # value, although the stored score equals that threshold
    down = [f for f in fin if F64(F32(sbar[f])) < sbar[f]]
    assert down, 'the case holds a face whose mean spread rounds down to f32'
    f = down[0]
    q = SR.landmark_scores(py, px, mu, None, ref, S, F64(F32(sbar[f])), None)
    assert q[2][f] & 1 and q[1][f, 0] == F32(sbar[f])


@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('shape', [(1, 1, 2, 2), (3, 10, 16, 16), (5, 30, 32, 16), (70, 64, 32, 32)])
def test_the_gpu_tests_cases_hold_what_they_say(shape, shared):
    """The cases tests/test_score_gpu.py runs the kernel on, checked here against their own description (score_reference asserts it)."""
    case, ref, ts, tr = SR.kernel_case_checked(*shape, shared=shared)
    assert ts is not None and (tr is None) == (shape[1] == 1)


def test_mu_out_is_a_bit_copy_or_the_quiet_nan():
    py, px, mu, ref = special_case()
    mu.view(np.uint32)[0, 0, 0] = 0x7fa00001                       # a signalling NaN with a payload in a face ... that is then unsure
    mu.view(np.uint32)[3, 1, 1] = 0x80000000                       # -0.0 in a sure face
    spread, score, qflags, mu_out, sbar, residual = SR.landmark_scores(py, px, mu, None, ref, S, None, None, 1)
    unsure = qflags != 0
    assert unsure[[0, 1, 2]].all() and not unsure[[3, 4, 5]].any()
    assert (mu_out.view(np.uint32)[unsure] == 0x7fc00000).all()
    assert np.array_equal(mu_out.view(np.uint32)[~unsure], mu.view(np.uint32)[~unsure])
    keep = SR.landmark_scores(py, px, mu, None, ref, S, None, None, 0)[3]
    assert np.array_equal(keep.view(np.uint32), mu.view(np.uint32)), 'blank = 0: bit copies, the NaN payload included'
    # a threshold blanks finite faces as well
    ts = np.sort(sbar[[3, 4, 5]])[1]
    r = SR.landmark_scores(py, px, mu, None, ref, S, ts, None, 1)
    assert (r[2][[3, 4, 5]] != 0).sum() == 1 and (r[3].view(np.uint32)[r[2] != 0] == 0x7fc00000).all()


def test_gated_step_loses_a_blanked_face_and_keeps_its_state():
    """The layering: NaN landmarks into the tested lost rule.  Face 1 is blanked on frame 1: its state, box and filter pairs stay."""
    import track_reference as TR
    F, K, h = 3, 6, 8
    hw = [(200, 220)]
    rows = np.array([[0, 10, 12, 90, 80], [0, 40, 50, 120, 140], [0, 5, 100, 75, 190]], dtype=np.int32)
    state = TR.new_state(F, K)
    py0, px0, mu0 = softmax_case(F, K, h, h, 2)
    a = SR.gated_step(py0, px0, mu0, rows, hw, state, S, (None, None), 0.5, (1.0, 0.05, 1.0), 25.0, True)
    assert (a['qflags'] == 0).all() and (a['flags'] & 1 == 0).all() and (a['score'][:, 1] == 0).all()
    py1, px1, mu1 = softmax_case(F, K, h, h, 3)
    sb = SR.landmark_scores(py1, px1, mu1, a['rows_next'], None, S)[4]
    ts = np.sort(sb)[1]                                            # the widest face fails
    worst = int(np.argmax(sb))
    before = state.copy()
    b = SR.gated_step(py1, px1, mu1, a['rows_next'], hw, state, S, (ts, None), 0.5, (1.0, 0.05, 1.0), 25.0, False)
    assert [int(q) for q in b['qflags']] == [1 if f == worst else 0 for f in range(F)]
    assert [int(q & 1) for q in b['flags']] == [1 if f == worst else 0 for f in range(F)]
    assert np.isnan(b['points'][worst]).all() and np.isfinite(np.delete(b['points'], worst, 0)).all()
    other = (worst + 1) % F
    assert np.array_equal(state[worst], before[worst]) and not np.array_equal(state[other], before[other])
    assert np.array_equal(b['rows_next'][worst, 1:], a['rows_next'][worst, 1:]), 'the next frame is cut with the same box'
    assert np.array_equal(b['mu'], mu1), 'the raw landmarks are what is reported'
    # frame 0 is never blanked, even when its bit is set
    st = TR.new_state(F, K)
    c = SR.gated_step(py0, px0, mu0, rows, hw, st, S, (1e-9, None), 0.5, None, 25.0, True)
    assert (c['qflags'] == 1).all() and (c['flags'] & 1 == 0).all() and np.isfinite(c['points']).all()


# ----------------------------------------------------------------------------------------------------------------------------
# the host side
# ----------------------------------------------------------------------------------------------------------------------------
def test_quality_gate_arguments():
    from imm_amd.quality import QualityGate
    g = QualityGate()
    assert g.max_spread is None and g.max_residual is None
    g = QualityGate(0.5, max_residual=0.25)
    assert (g.max_spread, g.max_residual) == (0.5, 0.25)
    for bad in (0, -1.0, float('nan'), float('inf'), 'wide'):
        with pytest.raises(ValueError):
            QualityGate(max_spread=bad)
        with pytest.raises(ValueError):
            QualityGate(max_residual=bad)


def test_quality_gate_fit():
    from imm_amd.quality import QualityGate
    rng = np.random.RandomState(0)
    sbar, resid = rng.uniform(0.1, 0.9, 50), rng.uniform(0.0, 0.3, 50)
    g = QualityGate.fit((sbar, resid), 0.9, 1.5)
    assert g.max_spread == 1.5 * float(np.quantile(sbar, 0.9)) and g.max_residual == 1.5 * float(np.quantile(resid, 0.9))
    g = QualityGate.fit((sbar.astype(np.float32), np.zeros(50, np.float32)), 1.0, 1.0)
    assert g.max_spread == float(np.float32(sbar).max()) and g.max_residual is None, 'all residuals 0: no reference was used'
    with pytest.raises(TypeError):
        QualityGate.fit((sbar, resid))                             # no defaults
    with pytest.raises(TypeError):
        QualityGate.fit((sbar, resid), 0.9)
    for q in (0.0, -0.1, 1.01, float('nan')):
        with pytest.raises(ValueError, match='quantile'):
            QualityGate.fit((sbar, resid), q, 1.5)
    for m in (0.99, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='margin'):
            QualityGate.fit((sbar, resid), 0.9, m)
    with pytest.raises(ValueError, match='finite'):
        QualityGate.fit((np.array([0.5, np.nan]), np.zeros(2)), 0.9, 1.5)
    with pytest.raises(ValueError):
        QualityGate.fit((np.zeros(0), np.zeros(0)), 0.9, 1.5)
    # a LandmarkQuality carries K, S and the heat-map side into the gate
    import torch
    from imm_amd.quality import LandmarkQuality
    n, K, h = 7, 10, 16
    score = torch.from_numpy(np.stack([sbar[:n], resid[:n]], 1).astype(np.float32))
    q = LandmarkQuality(torch.zeros(n, K, 2), torch.zeros(n, K), score, torch.tensor([0, 1, 2, 3, 0, 0, 0], dtype=torch.int32),
                        torch.zeros(n, h, K), torch.zeros(n, h, K), S)
    assert len(q) == n and torch.equal(q.sbar, score[:, 0]) and torch.equal(q.residual, score[:, 1])
    assert q.unsure.tolist() == [False, True, True, True, False, False, False]
    g = QualityGate.fit(q, 0.5, 2.0)
    assert g.max_spread == 2.0 * float(np.quantile(score[:, 0].numpy().astype(np.float64), 0.5)) and (g.K, g.S, g.heatmap) == (K, S, h)
    assert torch.equal(q.cpu().score, score)


def test_quality_gate_save_load_check(tmp_path):
    from imm_amd.alignment import LandmarkTemplate
    from imm_amd.quality import FORMAT, QualityGate
    assert FORMAT == 'imm-quality-gate-1'
    path = str(tmp_path / 'gate.npz')
    g = QualityGate(0.625, None, K=10, S=128, heatmap=16)
    g.save(path)
    with np.load(path, allow_pickle=False) as d:
        assert str(d['format']) == FORMAT and int(d['K']) == 10 and int(d['S']) == 128 and int(d['heatmap']) == 16
    r = QualityGate.load(path)
    assert (r.max_spread, r.max_residual, r.K, r.S, r.heatmap) == (0.625, None, 10, 128, 16)
    QualityGate(0.5, 0.1).save(path)
    r = QualityGate.load(path)
    assert (r.max_spread, r.max_residual, r.K, r.S, r.heatmap) == (0.5, 0.1, None, None, None)
    r.check(30, 64)                                                # a gate made by hand holds no K or S
    g.check(10, 128)
    with pytest.raises(ValueError, match='K = 10'):
        g.check(30, 128)
    with pytest.raises(ValueError, match='S = 128'):
        g.check(10, 64)

    class Det(object):
        K, S = 30, 128
    g.save(path)
    with pytest.raises(ValueError, match='K = 10'):
        QualityGate.load(path, detector=Det)
    # another npz is refused
    other = str(tmp_path / 'template.npz')
    LandmarkTemplate(np.random.RandomState(0).uniform(-0.5, 0.5, (10, 2)), 128).save(other)
    with pytest.raises(ValueError, match='not a quality gate'):
        QualityGate.load(other)
    np.savez(other, x=np.zeros(3))
    with pytest.raises(ValueError, match='not a quality gate'):
        QualityGate.load(other)


def test_plan_track_refuses_a_gate_of_the_wrong_type():
    from imm_amd.quality import QualityGate
    from imm_amd.tracking import plan_track
    frames = [np.zeros((40, 30, 3), np.uint8)] * 2
    boxes = [(0, 2, 3, 30, 25)]
    assert len(plan_track(frames, boxes, 4, gate=None)) == 5 == len(plan_track(frames, boxes, 4, gate=QualityGate(0.5)))
    for bad in (0.5, (0.5, None), 'gate.npz', dict(max_spread=0.5)):
        with pytest.raises(ValueError, match='QualityGate'):
            plan_track(frames, boxes, 4, gate=bad)
    from imm_amd.clip import plan_clip
    with pytest.raises(ValueError, match='QualityGate'):
        plan_clip(frames, boxes, [np.zeros((20, 20, 3), np.uint8)], gate=0.5)


def test_track_keeps_its_positional_signature():
    import torch
    from imm_amd.tracking import Track
    T, F, K = 3, 2, 4
    mu, boxes, flags = torch.zeros(T, F, K, 2), torch.zeros(T, F, 4, dtype=torch.int32), torch.tensor([[0, 1], [2, 3], [0, 0]], dtype=torch.int32)
    tr = Track(mu, mu, mu, boxes, flags)
    assert tr.keypoints is None and tr.spread is None and tr.score is None and tr.qflags is None
    assert tuple(tr.unsure.shape) == (T, F) and tr.unsure.dtype == torch.bool and not tr.unsure.any()
    kp = torch.zeros(T, F, 5, 2)
    tr = Track(mu, mu, mu, boxes, flags, kp)
    assert tr.keypoints is kp and not tr.unsure.any() and tr.lost.tolist() == [[False, True], [False, True], [False, False]]
    q = torch.tensor([[0, 1], [0, 0], [2, 3]], dtype=torch.int32)
    tr = Track(mu, mu, mu, boxes, flags, spread=torch.zeros(T, F, K), score=torch.zeros(T, F, 2), qflags=q)
    assert tr.unsure.tolist() == [[False, True], [False, False], [True, True]]
    c = tr.cpu()
    assert torch.equal(c.qflags, q) and tuple(c.spread.shape) == (T, F, K) and tuple(c.score.shape) == (T, F, 2)
