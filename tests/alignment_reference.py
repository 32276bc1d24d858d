"""float64 restatements of the alignment mathematics and conventions for the alignment tests, written from the definitions and
independent of imm_amd.alignment: the three fits (direct least squares / the bordered thin-plate-spline system, no F matrix), the
basis over the output grid, and the warp (q -> T(q) -> crop pixel -> source pixel -> bilinear with zero padding)."""
import numpy as np


def U(d2):
    d2 = np.asarray(d2, np.float64)
    out = np.zeros_like(d2)
    pos = d2 > 0
    out[pos] = d2[pos] * np.log(d2[pos])
    return out


def fit(t, mu, model, lam=0.0):
    """coef f64 [m3, 2] of the backward map template -> mu for one shape: rows U(|q - t_j|^2) (tps), then 1, q_y, q_x."""
    t, mu = np.asarray(t, np.float64), np.asarray(mu, np.float64)
    K = len(t)
    if model == 'affine':
        A = np.concatenate([np.ones((K, 1)), t], 1)
        return np.linalg.lstsq(A, mu, rcond=None)[0]
    if model == 'similarity':
        # min |a z + b - m|^2 over complex a, b: real unknowns (ar, ai, by, bx), rows y: ar ty - ai tx + by, x: ai ty + ar tx + bx
        A = np.zeros((2 * K, 4))
        A[0::2] = np.stack([t[:, 0], -t[:, 1], np.ones(K), np.zeros(K)], 1)
        A[1::2] = np.stack([t[:, 1], t[:, 0], np.zeros(K), np.ones(K)], 1)
        ar, ai, by, bx = np.linalg.lstsq(A, mu.reshape(-1), rcond=None)[0]
        return np.array([[by, bx], [ar, ai], [-ai, ar]])
    assert model == 'tps'
    L = np.zeros((K + 3, K + 3))
    L[:K, :K] = U(((t[:, None] - t[None]) ** 2).sum(-1)) + lam * np.eye(K)
    L[:K, K] = 1
    L[K, :K] = 1
    L[:K, K + 1:] = t
    L[K + 1:, :K] = t.T
    return np.linalg.solve(L, np.concatenate([mu, np.zeros((3, 2))]))


def tps_system_cond(t, lam=0.0):
    t = np.asarray(t, np.float64)
    K = len(t)
    L = np.zeros((K + 3, K + 3))
    L[:K, :K] = U(((t[:, None] - t[None]) ** 2).sum(-1)) + lam * np.eye(K)
    L[:K, K] = 1
    L[K, :K] = 1
    L[:K, K + 1:] = t
    L[K + 1:, :K] = t.T
    return np.linalg.cond(L)


def basis_at(t, q, tps):
    """[m3, P] at points q [P, 2]."""
    q = np.asarray(q, np.float64)
    rows = [U(((q - tj) ** 2).sum(-1)) for tj in np.asarray(t, np.float64)] if tps else []
    return np.stack(rows + [np.ones(len(q)), q[:, 0], q[:, 1]])


def grid(So):
    g = -1.0 + 2.0 * np.arange(So) / So
    return np.stack(np.meshgrid(g, g, indexing='ij'), -1).reshape(-1, 2)


def apply_map(t, coef, q):
    """T(q) f64 [P, 2] for coef [m3, 2]."""
    coef = np.asarray(coef, np.float64)
    return basis_at(t, q, len(coef) > 3).T @ coef


def warp(images, owner, geom, coef, t, S, So):
    """f64 [n, So, So, C]: the conventions of the issue restated.  images: list of HWC arrays; owner[b]: the image of row b."""
    q = grid(So)
    out = []
    for b, i in enumerate(owner):
        im = np.asarray(images[int(i)], np.float64)
        h, w = im.shape[:2]
        c = (apply_map(t, coef[b], q) + 1.0) / 2.0 * S
        g = np.asarray(geom[b], np.float64)
        sy, sx = g[0] + c[:, 0] * g[2], g[1] + c[:, 1] * g[3]
        y0, x0 = np.floor(sy), np.floor(sx)
        wy, wx = (sy - y0)[:, None], (sx - x0)[:, None]

        def tap(r, cc):
            ok = (r >= 0) & (r < h) & (cc >= 0) & (cc < w)
            v = im[np.clip(r, 0, h - 1).astype(np.int64), np.clip(cc, 0, w - 1).astype(np.int64)]
            return np.where(ok[:, None], v, 0.0)
        top = tap(y0, x0) * (1 - wx) + tap(y0, x0 + 1) * wx
        bot = tap(y0 + 1, x0) * (1 - wx) + tap(y0 + 1, x0 + 1) * wx
        out.append((top * (1 - wy) + bot * wy).reshape(So, So, -1))
    return np.stack(out)


def wholly_outside(images, owner, geom, coef, t, S, So):
    """bool [n, So, So]: all four taps of the pixel lie outside the photo."""
    q = grid(So)
    out = []
    for b, i in enumerate(owner):
        h, w = np.asarray(images[int(i)]).shape[:2]
        c = (apply_map(t, coef[b], q) + 1.0) / 2.0 * S
        g = np.asarray(geom[b], np.float64)
        sy, sx = g[0] + c[:, 0] * g[2], g[1] + c[:, 1] * g[3]
        y0, x0 = np.floor(sy), np.floor(sx)
        out.append(((y0 + 1 < 0) | (y0 >= h) | (x0 + 1 < 0) | (x0 >= w)).reshape(So, So))
    return np.stack(out)


def jittered_grid_template(K, seed):
    """K points on a jittered grid in [-0.7, 0.7]^2: well separated, never collinear."""
    rng = np.random.RandomState(seed)
    n = int(np.ceil(np.sqrt(K)))
    cells = rng.permutation(n * n)[:K]
    step = 1.4 / n
    yx = np.stack([cells // n, cells % n], 1).astype(np.float64)
    return -0.7 + (yx + 0.5 + rng.uniform(-0.3, 0.3, size=(K, 2))) * step


def smooth_photo(h, w, seed):
    """A smooth u8 photo: a sum of a few low-frequency sinusoids per channel."""
    rng = np.random.RandomState(seed)
    y, x = np.meshgrid(np.arange(h) / float(h), np.arange(w) / float(w), indexing='ij')
    im = np.zeros((h, w, 3))
    for ch in range(3):
        acc = np.zeros((h, w))
        for _ in range(4):
            fy, fx = rng.uniform(0.5, 3.0, 2)
            acc += rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * (fy * y + fx * x) + rng.uniform(0, 2 * np.pi))
        im[..., ch] = 127.5 + 110.0 * acc / np.abs(acc).max()
    return np.clip(np.rint(im), 0, 255).astype(np.uint8)
