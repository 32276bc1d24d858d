"""The tracking rule of include/imm_track.h restated in numpy f64, line by line after the header and in the operation order of
track_step_kernel (imm_amd/csrc/track.hip): every operation is one IEEE f64 operation (numpy scalars never fuse), sums run
k = 0 .. K - 1 from 0.0, np.fmin / np.fmax drop a NaN as fmin / fmax do, np.rint rounds ties to even.  The GPU tests compare the
kernel with this bit for bit; the CPU tests check it against hand-derived answers."""
import numpy as np

F64 = np.float64
F32 = np.float32


def state_size(K):
    return 5 + 6 * K


def source_pixel(mu, origin, dS, scale):
    t = F64(mu) + F64(1.0)
    t = t * F64(0.5)
    t = t * dS
    t = t * scale
    return origin + t


def alpha(c, fc):
    q = c * fc
    q = F64(1.0) / q
    q = F64(1.0) + q
    return F64(1.0) / q


def track_face(mu, box, hw, st, S, next_image, init, beta, min_cutoff, beta_e, d_cutoff, c, te, filter_off):
    """One face: mu f32 [K, 2], box int (image, y0, x0, y1, x1), hw int [n_images, 2], st f64 [5 + 6 K] (changed in place).
    Returns (points f32 [K, 2], points_smooth f32 [K, 2], next row int32 [5], geom f32 [4], flags int)."""
    mu = np.asarray(mu, dtype=F32)
    K = mu.shape[0]
    beta, min_cutoff, beta_e, d_cutoff, c, te = (F64(v) for v in (beta, min_cutoff, beta_e, d_cutoff, c, te))
    img = int(box[0])
    y0, x0, y1, x1 = (F64(int(v)) for v in box[1:])
    z0 = st[5:5 + 2 * K]
    xhat = st[5 + 2 * K:5 + 4 * K]
    dxhat = st[5 + 4 * K:5 + 6 * K]
    dS, dK = F64(S), F64(K)
    with np.errstate(all='ignore'):
        # 1. the geometry of this frame's box
        H, W = y1 - y0, x1 - x0
        sy, sx = F64(F32(H) / F32(S)), F64(F32(W) / F32(S))
        p = np.empty(2 * K, dtype=F64)
        for k in range(K):
            p[2 * k] = source_pixel(mu[k, 0], y0, dS, sy)
            p[2 * k + 1] = source_pixel(mu[k, 1], x0, dS, sx)
        # 2. start of a clip
        if init:
            ccy, ccx = (y0 + y1) * F64(0.5), (x0 + x1) * F64(0.5)
            st[0], st[1], st[2], st[3], st[4] = H, W, ccy, ccx, F64(1.0)
            for k in range(K):
                z0[2 * k], z0[2 * k + 1] = p[2 * k] - ccy, p[2 * k + 1] - ccx
                xhat[2 * k], xhat[2 * k + 1] = p[2 * k], p[2 * k + 1]
                dxhat[2 * k], dxhat[2 * k + 1] = 0.0, 0.0
        # 3. the similarity fit of z0 onto p
        finite = bool(np.isfinite(mu).all())
        points = p.astype(F32)
        mz0 = mz1 = mp0 = mp1 = F64(0.0)
        for k in range(K):
            mz0 = mz0 + z0[2 * k]
            mz1 = mz1 + z0[2 * k + 1]
            mp0 = mp0 + p[2 * k]
            mp1 = mp1 + p[2 * k + 1]
        mz0, mz1, mp0, mp1 = mz0 / dK, mz1 / dK, mp0 / dK, mp1 / dK
        den = ar = ai = F64(0.0)
        for k in range(K):
            u0, u1 = z0[2 * k] - mz0, z0[2 * k + 1] - mz1
            v0, v1 = p[2 * k] - mp0, p[2 * k + 1] - mp1
            den = den + (u0 * u0 + u1 * u1)
            ar = ar + (u0 * v0 + u1 * v1)
            ai = ai + (u0 * v1 - u1 * v0)
        a_r, a_i = ar / den, ai / den
        my = mp0 - (a_r * mz0 - a_i * mz1)
        mx = mp1 - (a_r * mz1 + a_i * mz0)
        ms = np.sqrt(a_r * a_r + a_i * a_i)
        lost = (not finite) or den == 0.0 or not (np.isfinite(my) and np.isfinite(mx) and np.isfinite(ms) and ms > 0.0)
        # 4. the box filter
        cy, cx, s = st[2], st[3], st[4]
        if not lost:
            cy = cy + beta * (my - cy)
            cx = cx + beta * (mx - cx)
            s = s + beta * (ms - s)
            st[2], st[3], st[4] = cy, cx, s
        # 5. the next box
        hn = np.fmin(np.fmax(np.rint(s * st[0]), F64(2.0)), F64(4194304.0))
        wn = np.fmin(np.fmax(np.rint(s * st[1]), F64(2.0)), F64(4194304.0))
        ny0 = np.fmin(np.fmax(np.rint(cy - hn * F64(0.5)), F64(-8388608.0)), F64(8388608.0))
        nx0 = np.fmin(np.fmax(np.rint(cx - wn * F64(0.5)), F64(-8388608.0)), F64(8388608.0))
        ny1, nx1 = ny0 + hn, nx0 + wn
        flags = 1 if lost else 0
        inside = False
        if 0 <= img < len(hw):
            sh, sw = F64(int(hw[img][0])), F64(int(hw[img][1]))
            inside = bool(ny0 < sh and ny1 > 0.0 and nx0 < sw and nx1 > 0.0)
        if not inside:
            flags |= 2
        # 6. the One-Euro filter
        if filter_off:
            smooth = points.copy()
        else:
            if not lost:
                rd = alpha(c, d_cutoff)
                th = te * H
                for i in range(2 * K):
                    if not np.isfinite(p[i]):
                        continue
                    xh, dh = xhat[i], dxhat[i]
                    dx = (p[i] - xh) / th
                    dh = dh + rd * (dx - dh)
                    fc = min_cutoff + beta_e * np.abs(dh)
                    xh = xh + alpha(c, fc) * (p[i] - xh)
                    xhat[i], dxhat[i] = xh, dh
            smooth = xhat.astype(F32)
        row = np.array([next_image, int(ny0), int(nx0), int(ny1), int(nx1)], dtype=np.int32)
        fS = F64(F32(S))
        geom = np.array([F32(ny0), F32(nx0), F32(hn / fS), F32(wn / fS)], dtype=F32)
    return points.reshape(K, 2), smooth.reshape(K, 2), row, geom, flags


def track_step(mu, boxes, hw, state, S, next_image, init, beta, one_euro=None, fps=25.0):
    """F faces: mu [F, K, 2], boxes int [F, 5], state f64 [F, 5 + 6 K] (changed in place).  one_euro: None (filter off) or
    (min_cutoff, beta, d_cutoff).  Returns (points, points_smooth f32 [F, K, 2], rows int32 [F, 5], geom f32 [F, 4], flags int32 [F])."""
    mc, be, dc = (1.0, 0.05, 1.0) if one_euro is None else one_euro
    c, te = 2.0 * np.pi / float(fps), 1.0 / float(fps)
    outs = [track_face(mu[f], boxes[f], hw, state[f], S, next_image, init, beta, mc, be, dc, c, te, one_euro is None)
            for f in range(len(boxes))]
    return (np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.stack([o[2] for o in outs]),
            np.stack([o[3] for o in outs]), np.array([o[4] for o in outs], dtype=np.int32))


def new_state(F, K):
    return np.zeros((F, state_size(K)), dtype=F64)
