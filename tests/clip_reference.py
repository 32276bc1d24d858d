"""The two rules of include/imm_clip.h restated in numpy, line by line after the header and in the operation order of
imm_amd/csrc/clip.hip: every operation is one IEEE operation of its type (numpy never fuses), np.fmin / np.fmax drop a NaN as fmin /
fmax do.  The GPU tests compare the kernels with this bit for bit; the CPU tests check it against the host functions it replaces
(generation.compose_inv_ramp, morphing.hull_inv_soft) and against the tracker's step 1 that it inverts."""
import numpy as np

F64 = np.float64
F32 = np.float32


def _ramp(feather, side):
    r = F64(feather) * side
    return F64(2.0) if r <= 0.5 else F64(1.0) / np.fmax(r, F64(0.5))


def _landmark(point, origin, scale, dS):
    v = F64(point) - origin
    v = v / scale
    v = v / dS
    v = v * F64(2.0)
    v = v - F64(1.0)
    if np.isfinite(v):
        v = np.fmin(np.fmax(v, F64(-1.0)), F64(1.0))
    return F32(v)


def clip_rows(boxes, track_flags, mu, points, S, feather, mask_feather):
    """imm_clip_rows: boxes int [F, 5], track_flags int [F], mu f32 [F, K, 2], points f32 [F, K, 2] or None, mask_feather f32 [F] or None
    -> (own f32 [F, K, 2], inv_ramp f32 [F, 2], inv_soft f32 [F] or None)."""
    boxes, mu = np.asarray(boxes), np.asarray(mu, dtype=F32)
    F, K = mu.shape[:2]
    own, inv_ramp = np.empty((F, K, 2), F32), np.empty((F, 2), F32)
    inv_soft = None if mask_feather is None else np.empty(F, F32)
    dS = F64(S)
    with np.errstate(all='ignore'):
        for f in range(F):
            y0, x0, y1, x1 = (F64(int(v)) for v in boxes[f, 1:])
            H, W = y1 - y0, x1 - x0
            inv_ramp[f] = F32(_ramp(feather, H)), F32(_ramp(feather, W))
            if mask_feather is not None:
                soft = F64(F32(mask_feather[f])) * np.fmin(H, W)
                inv_soft[f] = F32(F64(1.0) / np.fmax(F64(1.0), soft))
            if int(track_flags[f]) & 1:
                own[f] = np.nan
            elif points is None:
                own[f] = mu[f]
            else:
                sy, sx = F64(F32(H) / F32(S)), F64(F32(W) / F32(S))
                for k in range(K):
                    own[f, k, 0] = _landmark(F32(points[f][k][0]), y0, sy, dS)
                    own[f, k, 1] = _landmark(F32(points[f][k][1]), x0, sx, dS)
    return own, inv_ramp, inv_soft


def clip_ema(x, state, seen, skip, lost, alpha):
    """imm_clip_ema: x f32 [n, width], state f32 [n, width] and seen int32 [n] are changed in place; skip int [n], lost int [n] or None."""
    alpha = F32(alpha)
    assert x.dtype == F32 and state.dtype == F32 and seen.dtype == np.int32
    with np.errstate(all='ignore'):
        for i in range(len(x)):
            if int(skip[i]) != 0 or (lost is not None and int(lost[i]) & 1):
                continue
            if seen[i] == 0:
                state[i] = x[i]
            else:
                d = x[i] - state[i]
                m = alpha * d
                state[i] = state[i] + m
            x[i] = state[i]
            seen[i] = 1
    return x


def ema_frames(values, skips, losts, alpha):
    """The filter over a clip: values f32 [T, n, ...] (the raw values of every frame), skips int [T, n], losts int [T, n] -> the
    filtered values f32 [T, n, ...], from a fresh state."""
    values = np.asarray(values, dtype=F32)
    T, n = values.shape[:2]
    out = values.reshape(T, n, -1).copy()
    state, seen = np.zeros_like(out[0]), np.zeros(n, np.int32)
    for t in range(T):
        clip_ema(out[t], state, seen, skips[t], losts[t], alpha)
    return out.reshape(values.shape)
