"""The landmark-quality rule of include/imm_score.h restated in numpy f64, line by line after the header and in the operation order
of landmark_scores_kernel (imm_amd/csrc/score.hip): every operation is one IEEE f64 operation (numpy scalars never fuse), every sum
runs over ascending index from 0.0, np.fmax drops a NaN as fmax does.  The GPU tests compare the kernel with this bit for bit; the CPU
tests check it against hand-derived answers.  gated_track() is the tracker with a gate as a loop: this rule, then the step of
tests/track_reference.py on the gated landmarks.

What "bit for bit" means for a NaN: which NaN an arithmetic operation returns (sign, payload) is not fixed by IEEE 754, so same() takes
a NaN in the same place as equal in the computed outputs (spread, score, and what follows from them); mu_out, a copy or the constant
0x7fc00000, is compared as bits."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_reference as TR                      # noqa: E402

F64 = np.float64
F32 = np.float32
QNAN_BITS = np.uint32(0x7fc00000)
INF = float('inf')


def moment(q, m):
    """sum_i (double)q[i] * (d * d), d = (-1.0 + (2.0 * i) / (n - 1)) - m, for the K landmarks at once: q f32 [n, K], m f64 [K].  The K
    lanes are independent; an element-wise numpy operation is one IEEE operation per element, and the sum over i stays a loop."""
    n = q.shape[0]
    dn = F64(n - 1)
    v = np.zeros(q.shape[1], dtype=F64)
    for i in range(n):
        lin = F64(2.0) * F64(i)
        lin = lin / dn
        lin = F64(-1.0) + lin
        d = lin - m
        dd = d * d
        v = v + q[i].astype(F64) * dd
    return v


def score_face(py, px, mu, box, ref, S):
    """One face: py f32 [h, K], px f32 [w, K], mu f32 [K, 2], box int (image, y0, x0, y1, x1) or None, ref f64 [K, 2] or None.
    Returns (spread f64 [K], sbar f64, residual f64)."""
    K = mu.shape[0]
    dK = F64(K)
    with np.errstate(all='ignore'):
        # 1. spread
        vy = moment(py, mu[:, 0].astype(F64))
        vx = moment(px, mu[:, 1].astype(F64))
        spread = np.sqrt(vy + vx)
        sbar = F64(0.0)
        for k in range(K):
            sbar = sbar + spread[k]
        sbar = sbar / dK
        # 2. points
        p = np.empty(2 * K, dtype=F64)
        if box is None:
            for k in range(K):
                p[2 * k], p[2 * k + 1] = F64(mu[k, 0]), F64(mu[k, 1])
        else:
            y0, x0, y1, x1 = (F64(int(v)) for v in box[1:])
            H, W = y1 - y0, x1 - x0
            sy, sx = F64(F32(H) / F32(S)), F64(F32(W) / F32(S))
            for k in range(K):
                p[2 * k] = TR.source_pixel(mu[k, 0], y0, F64(S), sy)
                p[2 * k + 1] = TR.source_pixel(mu[k, 1], x0, F64(S), sx)
        # 3. shape residual
        if ref is None:
            return spread, sbar, F64(0.0)
        z0 = np.asarray(ref, dtype=F64).reshape(2 * K)
        mz0 = mz1 = mp0 = mp1 = F64(0.0)
        for k in range(K):
            mz0 = mz0 + z0[2 * k]
            mz1 = mz1 + z0[2 * k + 1]
            mp0 = mp0 + p[2 * k]
            mp1 = mp1 + p[2 * k + 1]
        mz0, mz1, mp0, mp1 = mz0 / dK, mz1 / dK, mp0 / dK, mp1 / dK
        den = ar = ai = pv = F64(0.0)
        for k in range(K):
            u0, u1 = z0[2 * k] - mz0, z0[2 * k + 1] - mz1
            v0, v1 = p[2 * k] - mp0, p[2 * k + 1] - mp1
            den = den + (u0 * u0 + u1 * u1)
            ar = ar + (u0 * v0 + u1 * v1)
            ai = ai + (u0 * v1 - u1 * v0)
            pv = pv + (v0 * v0 + v1 * v1)
        residual = F64('nan')
        if np.isfinite(den) and np.isfinite(pv) and den > 0.0 and pv > 0.0:
            num = ar * ar + ai * ai
            r2 = F64(1.0) - num / (den * pv)
            if np.isfinite(r2):
                residual = np.sqrt(np.fmax(r2, F64(0.0)))
    return spread, sbar, residual


def landmark_scores(py, px, mu, boxes, ref, S, max_spread=None, max_residual=None, blank=0):
    """F faces: py f32 [F, h, K], px f32 [F, w, K], mu f32 [F, K, 2], boxes int [F, 5] or None, ref None, f64 [K, 2] (one shape for
    all) or f64 [F, K, 2]; thresholds None = +inf.  Returns (spread f32 [F, K], score f32 [F, 2], qflags int32 [F], mu_out f32
    [F, K, 2], sbar f64 [F], residual f64 [F])."""
    py, px, mu = (np.asarray(a, dtype=F32) for a in (py, px, mu))
    F, K = mu.shape[:2]
    max_spread = F64(INF if max_spread is None else max_spread)
    max_residual = F64(INF if max_residual is None else max_residual)
    assert not (np.isnan(max_spread) or np.isnan(max_residual))
    if ref is not None:
        ref = np.asarray(ref, dtype=F64)
    spread, sbar, residual = np.empty((F, K), F64), np.empty(F, F64), np.empty(F, F64)
    for f in range(F):
        r = None if ref is None else (ref if ref.ndim == 2 else ref[f])
        spread[f], sbar[f], residual[f] = score_face(py[f], px[f], mu[f], None if boxes is None else boxes[f], r, S)
    # 4. flags, on the f64 values
    qflags = (~(sbar <= max_spread)).astype(np.int32) | ((~(residual <= max_residual)).astype(np.int32) << 1)
    # 5. gated landmarks, as bits
    bits = mu.view(np.uint32).copy()
    if blank:
        bits[qflags != 0] = QNAN_BITS
    with np.errstate(all='ignore'):
        score = np.stack([sbar.astype(F32), residual.astype(F32)], axis=1)
        return spread.astype(F32), score, qflags, bits.view(F32), sbar, residual


def same(got, want, what=''):
    """Equal bit for bit, a NaN in the same place counting as equal (see the module docstring)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == 'f':
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), '%s: NaN in other places (%d against %d)' % (what, gn.sum(), wn.sum())
        bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        g, w = np.where(gn, 0, got).view(bits), np.where(wn, 0, want).view(bits)
    else:
        g, w = got, want
    bad = np.argwhere(g != w)
    assert len(bad) == 0, '%s: %d of %d differ, first at %s: %r against %r' % (
        what, len(bad), g.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def same_bits(got, want, what=''):
    """Equal as bit patterns, NaNs included (mu_out)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    same(got.view(np.uint32), want.view(np.uint32), what)


def softmax_case(F, K, h, w, seed):
    """A random softmax per landmark and axis, mu its mean rounded to f32: what a pose head leaves.  (py [F, h, K], px [F, w, K], mu)."""
    rng = np.random.RandomState(seed)

    def marg(n):
        e = np.exp(rng.standard_normal((F, n, K)) * 2.0)
        return (e / e.sum(axis=1, keepdims=True)).astype(F32)
    py, px = marg(h), marg(w)
    ly, lx = np.linspace(-1, 1, h), np.linspace(-1, 1, w)
    mu = np.stack([(py.astype(F64) * ly[None, :, None]).sum(1), (px.astype(F64) * lx[None, :, None]).sum(1)], axis=-1).astype(F32)
    return py, px, mu


def kernel_case(F, K, h, w, seed, shared):
    """softmax_case with boxes and references, and the special faces planted where F allows: face 1 a NaN marginal, face 2 a NaN
    landmark, face 3 a degenerate shape (per-face references: its reference points coincide, den == 0; a shared reference: its
    landmarks coincide, pv == 0), face 4 an exact quarter-turned, halved, shifted copy of its reference (residual at rounding).
    shared: (py, px, mu, None, ref f64 [K, 2]); else (py, px, mu, boxes int32 [F, 5], state f64 [F, 5 + 6 K]) with the reference of
    face f in state[f, 5:5 + 2 K], as the tracker keeps it."""
    py, px, mu = softmax_case(F, K, h, w, seed)
    rng = np.random.RandomState(seed + 1000)
    if F >= 3:
        py[1, h // 2, K // 2] = np.nan
        mu[2, K - 1, 1] = np.nan
    if shared:
        ref = np.round(rng.uniform(-0.7, 0.7, (K, 2)) * 64) / 64
        if F >= 5:
            mu[3] = mu[3, 0]
            mu[4] = (np.stack([-ref[:, 1], ref[:, 0]], axis=1) * 0.5 + 0.125).astype(F32)
        return py, px, mu, None, ref
    side = rng.randint(20, 300, (F, 2))
    y0, x0 = rng.randint(-30, 250, F), rng.randint(-30, 250, F)
    boxes = np.stack([rng.randint(0, 3, F), y0, x0, y0 + side[:, 0], x0 + side[:, 1]], axis=1).astype(np.int32)
    state = rng.uniform(-50, 50, (F, 5 + 6 * K))
    if F >= 5:
        state[3, 5:5 + 2 * K] = np.tile([3.0, -7.0], K)              # small integers: their mean is exact, every u is 0
        boxes[4] = (1, -16, 32, 240, 288)                            # a square box of 256 = 2 S: source pixels are exact
        p = F64(-16.0) + (mu[4].astype(F64) + 1.0) * 0.5 * 128 * 2.0
        p[:, 1] += 48.0
        state[4, 5:5 + 2 * K] = (np.stack([p[:, 1], -p[:, 0]], axis=1) * 2.0 - 7.0).reshape(-1)
    return py, px, mu, boxes, state


def kernel_case_checked(F, K, h, w, shared):
    """kernel_case with its thresholds, two of the case's own f64 scores (the medians of the finite ones: those faces pass by equality),
    and the proof that the case holds what it says it holds: (case, ref [K, 2] or [F, K, 2], max_spread, max_residual)."""
    case = kernel_case(F, K, h, w, 7 * F + K + h, shared)
    py, px, mu, boxes, ref = case
    ref_np = ref if shared else ref[:, 5:5 + 2 * K].reshape(F, K, 2)
    sbar, residual = landmark_scores(py, px, mu, boxes, ref_np, 128)[4:]
    fin_s, fin_r = np.sort(sbar[np.isfinite(sbar)]), np.sort(residual[np.isfinite(residual)])
    ts = None if len(fin_s) == 0 else float(fin_s[len(fin_s) // 2])
    tr = None if len(fin_r) == 0 else float(fin_r[len(fin_r) // 2])
    q = landmark_scores(py, px, mu, boxes, ref_np, 128, ts, tr)[2]
    if K == 1:
        assert np.isnan(residual).all() and (q & 2).all(), 'one point has no scatter: den == 0'
    if F >= 3:
        assert q[1] & 1 and q[2] == 3 and np.isnan(sbar[1]) and np.isnan(residual[2])
        assert (sbar[np.isfinite(sbar)] == ts).any() and (residual[np.isfinite(residual)] == tr).any()
        assert ((q & 1) == 0).any() and ((q & 1) != 0).any()
    if F >= 5:
        assert np.isnan(residual[3]) and q[3] & 2 and residual[4] < 1e-6
    if F >= 70:
        assert ((q & 2) == 0).sum() > 10 and ((q & 2) != 0).sum() > 10
    return case, ref_np, ts, tr


def gated_step(py, px, mu, rows, hw, state, S, gate, beta, one_euro, fps, first, next_image=0):
    """One frame of the tracker with a gate = (max_spread, max_residual): this module's rule on the frame's marginals, landmarks and box
    rows, then track_reference's step on the gated landmarks; state f64 [F, 5 + 6 K] is changed in place.  The first frame is scored
    without a reference and not blanked; a later one is scored against z0 of the state and blanked."""
    K = mu.shape[1]
    ref = None if first else state[:, 5:5 + 2 * K].reshape(-1, K, 2).copy()
    spread, score, qflags, mu_g, sbar, _rs = landmark_scores(py, px, mu, rows, ref, S, gate[0], gate[1], 0 if first else 1)
    points, smooth, rows_next, _geom, flags = TR.track_step(mu_g, rows, hw, state, S, next_image, 1 if first else 0, beta, one_euro, fps)
    return dict(mu=np.asarray(mu, dtype=F32), points=points, points_smooth=smooth, boxes=np.array(rows[:, 1:], dtype=np.int32), flags=flags,
                spread=spread, score=score, qflags=qflags, sbar=sbar, rows_next=rows_next)


def gated_track(observe, sizes, boxes0, S, gate, beta, one_euro=None, fps=25.0):
    """The tracker with a gate as a loop over public calls.  observe(t, rows) -> (py [F, h, K], px [F, w, K], mu [F, K, 2]): what the
    pose program gives for frame t cut with the box rows int32 [F, 5] (image index 0); sizes[t] = (height, width) of frame t; boxes0
    int [F, 5]: the faces of frame 0.  Returns a dict of [T, ..] arrays: mu, points, points_smooth, boxes (the box each frame was cut
    with), flags, spread, score, qflags, sbar (f64)."""
    rows = np.array(boxes0, dtype=np.int32)
    F = len(rows)
    out, state = None, None
    for t, hw in enumerate(sizes):
        py, px, mu = observe(t, rows)
        if state is None:
            state = TR.new_state(F, mu.shape[1])
        step = gated_step(py, px, mu, rows, [tuple(hw)], state, S, gate, beta, one_euro, fps, t == 0)
        rows = step.pop('rows_next')
        out = out or {k: [] for k in step}
        for k, v in step.items():
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}
