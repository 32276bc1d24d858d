"""The re-enactment rule of include/imm_retarget.h restated in numpy f64, line by line after the header and in the operation order of
retarget_kernel (imm_amd/csrc/retarget.hip): every operation is one IEEE f64 operation (numpy scalars never fuse), sums run
k = 0 .. K - 1 from 0.0, np.fmin / np.fmax drop a NaN as fmin / fmax do.  The GPU tests compare the kernel with this bit for bit; the
CPU tests check it against hand-derived answers."""
import numpy as np

F64 = np.float64
F32 = np.float32
HELD = 1


def fit(z, p):
    """Step 3 of include/imm_track.h: z, p f64 [K, 2] -> (a_r, a_i, mz0, mz1, mp0, mp1, den)."""
    K = len(z)
    dK = F64(K)
    mz0 = mz1 = mp0 = mp1 = F64(0.0)
    for k in range(K):
        mz0 = mz0 + z[k, 0]
        mz1 = mz1 + z[k, 1]
        mp0 = mp0 + p[k, 0]
        mp1 = mp1 + p[k, 1]
    mz0, mz1, mp0, mp1 = mz0 / dK, mz1 / dK, mp0 / dK, mp1 / dK
    den = ar = ai = F64(0.0)
    for k in range(K):
        u0, u1 = z[k, 0] - mz0, z[k, 1] - mz1
        v0, v1 = p[k, 0] - mp0, p[k, 1] - mp1
        den = den + (u0 * u0 + u1 * u1)
        ar = ar + (u0 * v0 + u1 * v1)
        ai = ai + (u0 * v1 - u1 * v0)
    return ar / den, ai / den, mz0, mz1, mp0, mp1, den


def retarget_face(q, q0, driver_flags, m, prev, relative, rigid, gain):
    """One source face: q f32 [K, 2], q0 f64 [K, 2], m, prev f32 [K, 2] -> (out f32 [K, 2], flags int)."""
    q32, m32, prev = np.asarray(q, dtype=F32), np.asarray(m, dtype=F32), np.asarray(prev, dtype=F32)
    q, m, q0 = q32.astype(F64), m32.astype(F64), np.asarray(q0, dtype=F64)
    K = len(m)
    gain = F64(gain)
    with np.errstate(all='ignore'):
        held = bool(int(driver_flags) & 1)
        held = held or not (np.isfinite(q).all() and np.isfinite(q0).all() and np.isfinite(m).all())
        # 1. the driver's frame into the face's frame
        a_r, a_i, mq00, mq01, mm0, mm1, den_a = fit(q0, m)
        na = a_r * a_r + a_i * a_i
        held = held or den_a == 0.0 or na == 0.0
        # 2. head motion removed
        qt = q.copy()
        if not rigid:
            b_r, b_i, _z0, _z1, mq_0, mq_1, den_b = fit(q0, q)
            nb = b_r * b_r + b_i * b_i
            held = held or den_b == 0.0 or nb == 0.0
            for k in range(K):
                w0, w1 = q[k, 0] - mq_0, q[k, 1] - mq_1
                qt[k, 0] = mq00 + (b_r * w0 + b_i * w1) / nb
                qt[k, 1] = mq01 + (b_r * w1 - b_i * w0) / nb
        # 3, 4. the target and the value in front of the clamp
        o = np.empty((K, 2), dtype=F64)
        for k in range(K):
            if relative:
                d0, d1 = qt[k, 0] - q0[k, 0], qt[k, 1] - q0[k, 1]
                t0 = m[k, 0] + (a_r * d0 - a_i * d1)
                t1 = m[k, 1] + (a_r * d1 + a_i * d0)
            else:
                d0, d1 = qt[k, 0] - mq00, qt[k, 1] - mq01
                t0 = mm0 + (a_r * d0 - a_i * d1)
                t1 = mm1 + (a_r * d1 + a_i * d0)
            o[k, 0] = m[k, 0] + gain * (t0 - m[k, 0])
            o[k, 1] = m[k, 1] + gain * (t1 - m[k, 1])
        # 5. held
        held = held or not np.isfinite(o).all()
        if held:
            return prev.copy(), HELD
        return np.fmin(np.fmax(o, F64(-1.0)), F64(1.0)).astype(F32), 0


def retarget(q, anchor, driver_flags, m, prev, init, relative=True, rigid=True, gain=1.0):
    """n source faces: q f32 [K, 2], anchor f64 [K, 2] (set to q in place with init), driver_flags int, m, prev f32 [n, K, 2].
    Returns (out f32 [n, K, 2], flags int32 [n])."""
    q = np.asarray(q, dtype=F32)
    if init:
        anchor[...] = q.astype(F64)
    outs = [retarget_face(q, anchor, driver_flags, m[i], prev[i], relative, rigid, gain) for i in range(len(m))]
    return np.stack([o[0] for o in outs]), np.array([o[1] for o in outs], dtype=np.int32)


def retarget_clip(points, driver_flags, m, relative=True, rigid=True, gain=1.0):
    """A whole clip on the host: points f32 [T, K, 2] and driver_flags int [T] of the ONE driver face (a Track's points_smooth[:, 0]
    and flags[:, 0]), m f32 [n, K, 2] -> (landmarks f32 [T, n, K, 2], flags int32 [T, n]); a held face keeps the pose of the frame
    before (m on frame 0)."""
    m = np.asarray(m, dtype=F32)
    anchor = np.zeros(m.shape[1:], dtype=F64)
    prev, lms, fls = m, [], []
    for t in range(len(points)):
        prev, fl = retarget(points[t], anchor, driver_flags[t], m, prev, int(t == 0), relative, rigid, gain)
        lms.append(prev)
        fls.append(fl)
    return np.stack(lms), np.stack(fls)
