"""Alignment: photos warped so that their landmarks land on a fixed template, on the GPU (LandmarkDetector.align).

A template is K points t [K, 2], (y, x) in [-1, 1] of the detector's S x S frame (the mean landmark shape of a training split:
LandmarkTemplate.from_landmarks, scripts/test.py --save-template).  For a photo with landmarks mu_b, alignment needs the BACKWARD map
T_b: template frame -> the photo's S x S frame, with T_b(t_c) ~= mu_b,c.  Its control points are the template, the same for every
photo, so in all three models the coefficients are a fixed matrix times the photo's landmarks:

    coef_b = F . vec(mu_b)                 F f64 [2 m3, 2K], built once per (template, model, lam): fit_matrix
    T_b(q) = sum_j basis_j(q) coef_b[j]    basis: U(|q - t_j|^2) for j < m3 - 3 (tps only), then 1, q_y, q_x;  U(d2) = d2 log d2

    similarity  m3 = 3      rotation, isotropic scale, translation, no reflection: a = sum conj(t_c - t_mean)(mu_c - mu_mean) /
                            sum |t_c - t_mean|^2 over the points as complex numbers y + ix, T(q) = a (q - t_mean) + mu_mean
    affine      m3 = 3      least squares of mu on [1, t]
    tps         m3 = K + 3  thin-plate spline with smoothing lam >= 0: L^-1 [mu; 0] with L = [[U(|t_i - t_j|^2) + lam I, 1, t],
                            [1^T, 0, 0], [t^T, 0, 0]]; lam = 0 interpolates, lam -> inf tends to the affine fit

On the GPU imm_align_coeffs evaluates coef_b behind the pose head (captured in the bucket's graph) and imm_align_warp_u8 samples the
packed u8 photos once through T_b and the row's box geometry (keypoints()' conventions, so a keypoint and an aligned pixel name the
same place of the photo):

    output pixel (i, j) of So x So     q = (-1 + 2 i / So, -1 + 2 j / So)
    S x S frame                        c = (T_b(q) + 1) / 2 * S
    source photo                       s = (y0 + c_y sy, x0 + c_x sx),  geom (y0, x0, sy, sx) = keypoints.box_geometry
    value                              bilinear at s, taps floor(s) and floor(s) + 1, zeros outside the photo, f32 in [0, 255]

LandmarkDetector.unalign carries pixels the other way: aligned faces (edited or generated in the canonical frame) are pasted back into
their u8 photos through the inverse of the similarity or affine map (imm_unalign_maps, imm_unalign_u8; include/imm_unalign.h).

Unweighted fits only; no reflection handling; no forward TPS point map (Alignment.to_aligned and unalign serve similarity and affine)."""
import numpy as np

MODELS = ('similarity', 'affine', 'tps')
FORMAT = 'imm-landmark-template-1'
MAX_LANDMARKS = 64


def check_model(model, lam=0.0):
    if model not in MODELS:
        raise ValueError('model must be one of %s, got %r' % (', '.join(MODELS), model))
    lam = float(lam)
    if not lam >= 0.0 or not np.isfinite(lam):
        raise ValueError('lam must be finite and >= 0, got %r' % (lam,))
    if lam and model != 'tps':
        raise ValueError('lam is the smoothing of the tps model; %s takes none' % model)
    return lam


def n_basis(model, K):
    """m3: basis functions (coefficient rows) of a model's map."""
    return int(K) + 3 if model == 'tps' else 3


def tps_kernel(d2):
    """U(d2) = d2 log d2 of squared distances, U(0) = 0."""
    d2 = np.asarray(d2, dtype=np.float64)
    return np.where(d2 > 0, d2 * np.log(np.where(d2 > 0, d2, 1.0)), 0.0)


def _as_complex(p):
    return p[..., 0] + 1j * p[..., 1]


def fit_similarity(src, dst):
    """(a, b) complex with a * z + b the least-squares similarity (no reflection) taking the points src [K, 2] to dst [K, 2], points
    as complex numbers y + ix."""
    zs, zd = _as_complex(np.asarray(src, np.float64)), _as_complex(np.asarray(dst, np.float64))
    sc = zs - zs.mean()
    den = float((np.abs(sc) ** 2).sum())
    if den <= 0:
        raise ValueError('a shape whose points all coincide has no similarity fit')
    a = (np.conj(sc) * (zd - zd.mean())).sum() / den
    return a, zd.mean() - a * zs.mean()


class LandmarkTemplate(object):
    """K template points (y, x) in [-1, 1] of the S x S landmark frame.  ValueError when two points coincide (distance < 1e-6) or all
    of them are collinear ([1, t] has rank < 3): exactly the cases in which the tps system at lam = 0 or the affine normal matrix is
    singular, kept away from the kernels here."""

    def __init__(self, points, image_size, dataset='', checkpoint=''):
        t = np.array(points, dtype=np.float64)
        if t.ndim != 2 or t.shape[1] != 2 or not 3 <= t.shape[0] <= MAX_LANDMARKS:
            raise ValueError('template points must be [K, 2] with 3 <= K <= %d, got %s' % (MAX_LANDMARKS, t.shape))
        if not np.isfinite(t).all():
            raise ValueError('template points must be finite')
        d = np.sqrt(((t[:, None] - t[None]) ** 2).sum(-1)) + np.eye(len(t))
        if d.min() < 1e-6:
            i, j = np.unravel_index(np.argmin(d), d.shape)
            raise ValueError('template points %d and %d coincide' % (i, j))
        sv = np.linalg.svd(np.concatenate([np.ones((len(t), 1)), t], axis=1), compute_uv=False)
        if sv[-1] <= 1e-9 * sv[0]:
            raise ValueError('the template points are collinear')
        self.points, self.K, self.S = t, t.shape[0], int(image_size)
        self.dataset, self.checkpoint = str(dataset), str(checkpoint)
        self._cache = {}

    # ------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_landmarks(cls, mu, image_size, procrustes_iterations=3, dataset='', checkpoint=''):
        """The mean shape of landmarks mu [N, K, 2].  procrustes_iterations = 0: the plain mean.  Otherwise that many rounds of
        similarity-aligning every shape to the current mean and re-averaging; after each round the mean is put back at the plain
        mean's centroid and orientation and at the shapes' mean size (root sum of squared distances to the centroid), so rotated,
        scaled and shifted copies of one shape give that shape back at their average pose instead of a shrunken one."""
        mu = np.asarray(mu, dtype=np.float64)
        if mu.ndim != 3 or mu.shape[2] != 2 or mu.shape[0] < 1:
            raise ValueError('mu must be [N, K, 2], got %s' % (mu.shape,))
        rounds = int(procrustes_iterations)
        if rounds < 0:
            raise ValueError('procrustes_iterations must be >= 0')
        plain = mu.mean(axis=0)
        if rounds == 0:
            return cls(plain, image_size, dataset, checkpoint)
        z = _as_complex(mu)                                            # [N, K]
        zc = z - z.mean(axis=1, keepdims=True)
        den = (np.abs(zc) ** 2).sum(axis=1)
        if den.min() <= 0:
            raise ValueError('a shape whose points all coincide cannot be aligned')
        size = float(np.sqrt(den).mean())
        pz = _as_complex(plain)
        pc = pz - pz.mean()
        ref = pz
        for _ in range(rounds):
            rc = ref - ref.mean()
            a = (np.conj(zc) * rc[None]).sum(axis=1) / den                # every shape onto the current mean
            m = (a[:, None] * zc).mean(axis=0)                            # centred
            rot = (np.conj(m) * pc).sum()
            norm = np.sqrt((np.abs(m) ** 2).sum())
            if abs(rot) <= 0 or norm <= 0:
                raise ValueError('the mean shape degenerated to a point')
            ref = m * (rot / abs(rot)) * (size / norm) + pz.mean()
        return cls(np.stack([ref.real, ref.imag], axis=1), image_size, dataset, checkpoint)

    # ------------------------------------------------------------------------------------------------------------------------
    def fit(self, mu, model='similarity', lam=0.0):
        """coef f64 [..., m3, 2] of the backward map for landmarks mu [..., K, 2] (host; the arithmetic F stands for)."""
        F = self.fit_matrix(model, lam)
        mu = np.asarray(mu, dtype=np.float64)
        if mu.shape[-2:] != (self.K, 2):
            raise ValueError('mu must be [..., %d, 2], got %s' % (self.K, mu.shape))
        return (mu.reshape(mu.shape[:-2] + (2 * self.K,)) @ F.T).reshape(mu.shape[:-2] + (F.shape[0] // 2, 2))

    def fit_matrix(self, model='similarity', lam=0.0):
        """F f64 [2 m3, 2K]: coef.reshape(-1) = F . mu.reshape(-1) for mu [K, 2], coef [m3, 2] ((y, x) per basis function)."""
        lam = check_model(model, lam)
        key = ('F', model, lam)
        if key not in self._cache:
            t, K = self.points, self.K
            if model == 'similarity':
                z = _as_complex(t)
                zc = z - z.mean()
                den = (np.abs(zc) ** 2).sum()
                F = np.zeros((6, 2 * K))
                for i in range(2 * K):                    # linear in mu: the columns are the fits of the unit vectors
                    e = np.zeros(2 * K)
                    e[i] = 1.0
                    m = _as_complex(e.reshape(K, 2))
                    a = (np.conj(zc) * (m - m.mean())).sum() / den
                    b = m.mean() - a * z.mean()
                    # T(q) = a q + b with q = q_y + i q_x: rows 1, q_y, q_x of (y, x) coefficients
                    F[:, i] = [b.real, b.imag, a.real, a.imag, -a.imag, a.real]
            elif model == 'affine':
                A = np.concatenate([np.ones((K, 1)), t], axis=1)
                F = np.kron(np.linalg.solve(A.T @ A, A.T), np.eye(2))
            else:
                Lm = np.zeros((K + 3, K + 3))
                Lm[:K, :K] = tps_kernel(((t[:, None] - t[None]) ** 2).sum(-1)) + lam * np.eye(K)
                Lm[:K, K] = Lm[K, :K] = 1.0
                Lm[:K, K + 1:] = t
                Lm[K + 1:, :K] = t.T
                F = np.kron(np.linalg.solve(Lm, np.eye(K + 3))[:, :K], np.eye(2))
            self._cache[key] = F
        return self._cache[key]

    def basis_at(self, model, q):
        """The basis functions at template-frame points q [..., 2]: f64 [m3, ...]."""
        check_model(model)
        q = np.asarray(q, dtype=np.float64)
        rows = []
        if model == 'tps':
            rows = list(tps_kernel(((q[None] - self.points.reshape((self.K,) + (1,) * (q.ndim - 1) + (2,))) ** 2).sum(-1)))
        return np.stack(rows + [np.ones(q.shape[:-1]), q[..., 0], q[..., 1]])

    def basis(self, model, out_size):
        """f64 [m3, So * So]: the basis over the output grid q = (-1 + 2 i / So, -1 + 2 j / So), pixel (i, j) at column i * So + j."""
        So = int(out_size)
        g = -1.0 + 2.0 * np.arange(So, dtype=np.float64) / So
        q = np.stack(np.meshgrid(g, g, indexing='ij'), axis=-1).reshape(-1, 2)
        return self.basis_at(model, q)

    def check(self, n_landmarks, image_size):
        if self.K != int(n_landmarks) or self.S != int(image_size):
            raise ValueError('template of K = %d landmarks at S = %d, the detector has K = %d, S = %d' % (
                self.K, self.S, int(n_landmarks), int(image_size)))

    def save(self, path):
        with open(path, 'wb') as f:
            np.savez(f, format=np.array(FORMAT), points=self.points, K=np.int64(self.K), S=np.int64(self.S),
                     dataset=np.array(self.dataset), checkpoint=np.array(self.checkpoint))

    @classmethod
    def load(cls, path, detector=None):
        """A saved template; with `detector`, ValueError unless its K and S are the detector's."""
        with np.load(path, allow_pickle=False) as d:
            if 'format' not in d or str(d['format']) != FORMAT:
                raise ValueError('%s is not a landmark template file' % path)
            tpl = cls(d['points'], int(d['S']), str(d['dataset']), str(d['checkpoint']))
            if tpl.K != int(d['K']):
                raise ValueError('%s: K = %d but %d points' % (path, int(d['K']), tpl.K))
        if detector is not None:
            tpl.check(detector.K, detector.S)
        return tpl


def unalign_inv_ramp(feather, out_size):
    """The reciprocal of the paste's edge ramp, feather * So aligned pixels wide, as the f32 value imm_unalign_u8 takes; 2 where that
    width is <= 0.5 pixels (every weight is then 1: a hard paste; feather == 0 always is).  feather: checked by the caller."""
    ramp = float(feather) * int(out_size)
    return 2.0 if ramp <= 0.5 else float(np.float32(1.0 / ramp))


class Alignment(object):
    """What align(return_transform=True) returns next to the images: coef f32 [n, m3, 2] (the backward maps), geom f32 [n, 4]
    ((y0, x0, sy, sx) per row), mu f32 [n, K, 2] (tensors on the detector's device, or arrays), the model, lam, the template and the
    output size; for u8 photo input also rows int32 [n, 5], the box rows (image, y0, x0, y1, x1) the faces were cut from (a host
    array; None for a tensor batch), which LandmarkDetector.unalign needs to find each row's photo."""

    def __init__(self, coef, geom, mu, model, lam, template, out_size, rows=None):
        self.coef, self.geom, self.mu = coef, geom, mu
        self.model, self.lam, self.template, self.out_size = model, float(lam), template, int(out_size)
        self.rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 5)

    @staticmethod
    def _host(a):
        return np.asarray(a.detach().cpu().numpy() if hasattr(a, 'detach') else a, dtype=np.float64)

    def to_source(self, points_aligned):
        """Pixel coordinates (i, j) [n, P, 2] (or [P, 2] for every row) of the aligned images -> (y, x) source pixels f64 [n, P, 2]."""
        coef, geom = self._host(self.coef), self._host(self.geom)
        p = np.asarray(points_aligned, dtype=np.float64)
        if p.ndim == 2:
            p = np.broadcast_to(p, (len(coef),) + p.shape)
        if p.ndim != 3 or p.shape[0] != len(coef) or p.shape[2] != 2:
            raise ValueError('points must be [n, P, 2] or [P, 2], got %s' % (p.shape,))
        q = -1.0 + 2.0 * p / self.out_size
        basis = self.template.basis_at(self.model, q)                        # [m3, n, P]
        v = np.einsum('jnp,njc->npc', basis, coef)
        c = (v + 1.0) / 2.0 * self.template.S
        return geom[:, None, :2] + c * geom[:, None, 2:]

    def to_aligned(self, points_source):
        """(y, x) source pixels [n, P, 2] -> pixel coordinates of the aligned images f64 [n, P, 2], by the inverse 2 x 3 map
        (similarity and affine; a thin-plate spline has no closed inverse: NotImplementedError)."""
        if self.model == 'tps':
            raise NotImplementedError('to_aligned serves the similarity and affine models; the tps map is not inverted')
        coef, geom = self._host(self.coef), self._host(self.geom)
        s = np.asarray(points_source, dtype=np.float64)
        if s.ndim == 2:
            s = np.broadcast_to(s, (len(coef),) + s.shape)
        if s.ndim != 3 or s.shape[0] != len(coef) or s.shape[2] != 2:
            raise ValueError('points must be [n, P, 2] or [P, 2], got %s' % (s.shape,))
        c = (s - geom[:, None, :2]) / geom[:, None, 2:]
        v = 2.0 * c / self.template.S - 1.0
        # v = coef[0] + q_y coef[1] + q_x coef[2]  =>  q = (v - coef[0]) . inv([coef[1]; coef[2]])
        q = np.einsum('npc,ncd->npd', v - coef[:, None, 0], np.linalg.inv(coef[:, 1:3]))
        return (q + 1.0) / 2.0 * self.out_size

