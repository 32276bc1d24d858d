"""Two faces blended in shape and texture from their own pixels: the host side of LandmarkDetector.morph (include/imm_morph.h states
the rule).

transfer(), repose() with pose photos and reenact() bring a second face into a photograph through the generator: a 300-pixel face comes
back as an up-sampled 128-pixel render.  morph() works on the pixels of the two photographs instead.  Per row there is a face of its
own (a box in one of the photos) and a donor face (a box in one of the donor photos), and two numbers in [0, 1]: `shape` moves the
landmarks from the face's own (0) to the donor's (1), `texture` mixes the pixels from the face's own (0) to the donor's (1).  The blended
landmarks p are the control points (with warp()'s border anchors) of TWO displacement splines, fitted by one imm_warp_fit launch: one
carries p back to the face's own landmarks, the other to the donor's, so every pixel of the box finds its place in both photographs and
takes the mix of what lies there.  shape = texture = t is the morph at t, shape = 0 with texture = 1 the donor's face swapped in place,
texture = 0 warp() towards the blended pose.

morph(colour=...) adds colour matching (include/imm_colour.h states the rule): per row and channel the mean and the spread of the face's
pixels and of the donor's pixels, each over the ellipse inscribed in its box, give a gain and an offset that the donor's sample takes in
front of the mix, so that a donor photographed in other light arrives in the face's tone.

morph(mask='hull') pastes only the face (include/imm_hull.h states the rule): the convex hull of the row's blended landmarks, grown about
their centroid by `grow` and softened inwards over mask_feather * min(H, W) pixels, multiplies the box's edge ramp, so the donor's
background, hair and collar stay out of the photo; pixels outside the hull skip the spline altogether.

morph(mask='hull', seamless=...) hides the seam of the mask (include/imm_seam.h states the rule): the colour differences between the
photo and the morph's mix at `ring` samples of the mask's outline are weighed, per pixel and in closed form, by the pixel's mean-value
coordinates in that ring, and the share `seamless` of that smooth correction is added to the mix, so that the donor's pixels keep
their detail and meet the photo's own values on the outline.

Here: the pose blend in the kernel's f32 order, the argument checks of morph() and PhotoMorph, what morph(return_transform=True) returns.
Nothing here needs a GPU."""
import numpy as np

from .inference import _Plan
from .warping import _host, check_spline, displacement

MAX_ROWS = 32767               # rows of one morph() call: imm_warp_fit takes 2 n <= 65535 rows
MASKS = (None, 'hull')         # morph(mask=...)
MAX_GROW = 16.0                # grow of morph(mask='hull') lies in (0, 16]
MIN_RING, MAX_RING = 16, 256   # ring of morph(seamless=...): the samples on the outline of the mask
COLOUR_MAX_AREA = 1 << 30      # H * W of a box whose colour statistics are taken: imm_colour_stats_u8's integer ellipse test stays in 64 bits


def blend_poses(mu_a, mu_b, shape):
    """p = (1 - s) * mu_a + s * mu_b, f32 [n, K, 2], in imm_morph_poses' order (numpy rounds every f32 operation separately): mu_a, mu_b
    [n, K, 2] and shape [n] are read as f32.  s = 0 gives mu_a and s = 1 gives mu_b as values; a NaN input gives NaN."""
    a, b = np.asarray(mu_a, dtype=np.float32), np.asarray(mu_b, dtype=np.float32)
    s = np.asarray(shape, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 2 or b.shape != a.shape or s.shape != a.shape[:1]:
        raise ValueError('mu_a and mu_b must be [n, K, 2] and shape [n], got %s, %s and %s' % (a.shape, b.shape, s.shape))
    s = s[:, None, None]
    with np.errstate(invalid='ignore', over='ignore'):
        wa = np.float32(1.0) - s
        ta, tb = wa * a, s * b
        return ta + tb


def _share(value, n, name, bounds=None):
    """A scalar or [n] in [0, 1] -> f32 [n].  bounds = (interval as text, test of the f64 values, what the number is): that interval
    instead."""
    v = np.asarray(value, dtype=np.float64)
    if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != n):
        raise ValueError('%s must be a number or one per row [%d], got shape %s' % (name, n, v.shape))
    v = np.broadcast_to(v, (n,))
    if bounds is None:
        if not (np.isfinite(v).all() and (v >= 0.0).all() and (v <= 1.0).all()):
            raise ValueError('%s must be finite and lie in [0, 1] (0: the face itself, 1: the donor), got %r' % (name, value))
    else:
        interval, inside, what = bounds
        if not (np.isfinite(v).all() and inside(v).all()):
            raise ValueError('%s must be finite and lie in %s (%s), got %r' % (name, interval, what, value))
    return np.ascontiguousarray(v, dtype=np.float32)


def _given_landmarks(lm, counts, K, name):
    """landmarks= / donor_landmarks=: f32 [n, K, 2] (or one of the other counts allowed) as a tensor; a host tensor must be finite (a device
    tensor is not read back: its rows are judged by the fit)."""
    import torch
    from .inference import check_landmarks
    t = check_landmarks(lm, counts, K, name)
    if not t.is_cuda and not bool(torch.isfinite(t).all()):
        raise ValueError('%s must be finite' % name)
    return t


def check_max_gain(max_gain):
    """max_gain of morph(colour=...): finite and >= 1 -> float."""
    try:
        g = float(max_gain)
    except (TypeError, ValueError):
        raise ValueError('max_gain must be a number, got %r' % (max_gain,))
    if not (g >= 1.0 and g - g == 0.0):
        raise ValueError('max_gain must be finite and >= 1 (the ratio of the spreads is kept in [1 / max_gain, max_gain]), got %r' % (max_gain,))
    return g


def check_grow(grow, n):
    """grow of mask='hull' (morph, redact): a number or one per row in (0, 16] -> f32 [n]."""
    return _share(grow, n, 'grow', ('(0, %g]' % MAX_GROW, lambda v: (v > 0.0) & (v <= MAX_GROW),
                                    'the factor by which the landmark hull is grown about its centroid'))


def check_mask_feather(mask_feather, n):
    """mask_feather of mask='hull' (morph, redact): a number or one per row in [0, 1] -> f32 [n]."""
    return _share(mask_feather, n, 'mask_feather', ('[0, 1]', lambda v: (v >= 0.0) & (v <= 1.0),
                                                    'the share of the box\'s shorter side over which the mask softens inwards'))


def hull_inv_soft(rows, mask_feather):
    """inv_soft f32 [n] of morph(mask='hull'): (float)(1 / max(1, mask_feather * min(H, W))), formed in f64 from the f32 mask_feather
    widened: the hull's weight is 0 on the grown hull's edge and 1 that many pixels (at least one) inside it."""
    rows = np.asarray(rows)
    side = np.minimum(rows[:, 3].astype(np.int64) - rows[:, 1], rows[:, 4].astype(np.int64) - rows[:, 2]).astype(np.float64)
    soft = np.maximum(1.0, np.asarray(mask_feather, dtype=np.float32).astype(np.float64) * side)
    return (1.0 / soft).astype(np.float32)


def check_ring(ring):
    """ring of morph(seamless=...): an int in [16, 256] -> int."""
    if isinstance(ring, bool) or not isinstance(ring, (int, np.integer)) or not MIN_RING <= int(ring) <= MAX_RING:
        raise ValueError('ring must be an int in [%d, %d] (the samples on the outline of the mask), got %r' % (MIN_RING, MAX_RING, ring))
    return int(ring)


def seam_dirs(ring):
    """dirs f64 [ring, 2] of imm_seam_fit: (cos, sin) of 2 pi s / ring, the (y, x) direction of sample s, formed here so that no
    transcendental function runs on the device."""
    a = 2.0 * np.pi * np.arange(ring, dtype=np.float64) / np.float64(ring)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1))


def seam_field(ring, diff, H, W):
    """The membrane of imm_morph_seam_u8 over a box of H x W pixels, f32 [H, W, 3], in the rule's f32 order (include/imm_seam.h): ring
    f32 [B, 2] (box-relative pixels), diff f32 [B, 3].  Per pixel the mean of the diffs weighed by the pixel's mean-value coordinates in
    the ring; the diff of the lowest sample the pixel lies on; 0 where the sum of the weights is not positive or a sum is not finite."""
    f32 = np.float32
    rg, df = np.asarray(ring, dtype=f32), np.asarray(diff, dtype=f32)
    B = len(rg)
    rr, cc = np.arange(max(H, 0), dtype=f32)[:, None], np.arange(max(W, 0), dtype=f32)[None, :]
    with np.errstate(all='ignore'):
        py, px = (rg[:, 0, None, None] - rr) + f32(0) * cc, (rg[:, 1, None, None] - cc) + f32(0) * rr      # [B, H, W]
        ln = np.sqrt(py * py + px * px)
        nxt = np.roll(np.arange(B), -1)
        cr, dt = py * px[nxt] - px * py[nxt], py * py[nxt] + px * px[nxt]
        th = cr / (ln * ln[nxt] + dt)
        R, Ws = np.zeros(py.shape[1:] + (3,), f32), np.zeros(py.shape[1:], f32)
        for k in range(B):
            w = (th[k - 1] + th[k]) / ln[k]
            R = R + w[..., None] * df[k]
            Ws = Ws + w
        ok = (Ws > 0) & np.isfinite(Ws) & np.isfinite(R).all(axis=-1)
        out = np.where(ok[..., None], R / np.where(ok, Ws, f32(1))[..., None], f32(0)).astype(f32)
    on = ln == 0
    first = np.argmax(on, axis=0)
    hit = on.any(axis=0)
    out[hit] = df[first[hit]]
    assert out.dtype == f32
    return out


class MorphPlan(_Plan):
    """What plan_morph returns, by name: photos and donors (decoded u8 arrays), rows and donor_rows int32 [n, 5] (ONE donor row is repeated
    for every face), donor_rows_given (the donor rows as given: what detector.landmarks(donors, .) is asked for), shape and texture f32
    [n], feather, anchors (per side), lam, M (control points), landmarks and donor_landmarks (None or f32 tensors), colour f32 [n] and
    max_gain; the mask's: mask (None or 'hull'), grow f32 [n], mask_feather f32 [n] and inv_soft f32 [n] (hull_inv_soft of the rows); and
    the membrane's: seamless f32 [n] and ring (an int)."""
    FIELDS = ('photos', 'rows', 'donors', 'donor_rows', 'donor_rows_given', 'shape', 'texture', 'feather', 'anchors', 'lam', 'M', 'landmarks',
              'donor_landmarks', 'colour', 'max_gain', 'mask', 'grow', 'mask_feather', 'inv_soft', 'seamless', 'ring')


def plan_morph(photos, donors, boxes, donor_boxes, shape, texture, feather, K, anchors=2, lam=0.0, landmarks=None, donor_landmarks=None,
               colour=0.0, max_gain=2.0, mask=None, grow=1.25, mask_feather=0.1, seamless=0.0, ring=128):
    """morph()'s arguments checked on the host, before anything reaches the device: (photos as decoded u8 arrays, box rows int32 [n, 5],
    donor photos as decoded u8 arrays, donor box rows int32 [n, 5] (ONE donor row is repeated for every face), the donor rows as given
    (what detector.landmarks(donors, .) is asked for), shape f32 [n], texture f32 [n], feather, m, lam, M, landmarks, donor_landmarks,
    colour f32 [n], max_gain).  colour: a number or one per row in [0, 1]; with any colour > 0 a box of more than 2^30 pixels on either
    side is refused (imm_colour_stats_u8 would count nothing there).
    photos / boxes and donors / donor_boxes in generation.plan_repose's forms (lists of u8 arrays; box rows, by default one whole-photo
    box per photo).  texture=None: texture = shape.  landmarks / donor_landmarks: None or f32 [n, K, 2] tensors (donor_landmarks may have
    one row when there is one donor row).
    mask: None or 'hull'; grow: a number or one per row in (0, 16]; mask_feather: likewise in [0, 1].  They are checked whatever mask is,
    and returned as attributes of the result (a MorphPlan).
    seamless: a number or one per row in [0, 1], the share of the mean-value correction that is added; ring: an int in [16, 256].  Both
    are checked whatever their value and returned as attributes; any seamless > 0 needs mask='hull'."""
    from .generation import NEEDS_U8, check_feather
    if mask not in MASKS:
        raise ValueError("mask must be None or 'hull', got %r" % (mask,))
    from .inference import photos_and_rows
    m, lam, _strength, M = check_spline(anchors, lam, 1.0, K)
    feather = check_feather(feather)
    needs, needs_donors = 'photos: %s' % NEEDS_U8, 'donors: %s' % NEEDS_U8
    photos, rows = photos_and_rows(photos, boxes, needs, needs, limit=(
        MAX_ROWS, 'a morph serves at most %d rows a call (one fit over twice as many), got %%d' % MAX_ROWS))
    donors, drows = photos_and_rows(donors, donor_boxes, needs_donors, needs_donors)
    n, n_d = len(rows), len(drows)
    if n_d not in (n, 1):
        raise ValueError('%d donors for %d faces: give one per face, or one for all' % (n_d, n))
    shape = _share(shape, n, 'shape')
    texture = shape.copy() if texture is None else _share(texture, n, 'texture')
    if landmarks is not None:
        landmarks = _given_landmarks(landmarks, (n,), K, 'landmarks')
    if donor_landmarks is not None:
        donor_landmarks = _given_landmarks(donor_landmarks, (n,) if n_d == n else (n, 1), K, 'donor_landmarks')
    full = np.ascontiguousarray(np.broadcast_to(drows, (n, 5)) if n_d != n else drows, dtype=np.int32)
    colour, max_gain = _share(colour, n, 'colour'), check_max_gain(max_gain)
    if colour.any():
        for name, rw in (('boxes', rows), ('donor_boxes', full)):
            area = (rw[:, 3].astype(np.int64) - rw[:, 1]) * (rw[:, 4].astype(np.int64) - rw[:, 2])
            if (area > COLOUR_MAX_AREA).any():
                raise ValueError('%s: row %d has %d pixels; colour matching serves boxes of at most 2^30' % (
                    name, int(np.argmax(area > COLOUR_MAX_AREA)), int(area.max())))
    grow, mask_feather = check_grow(grow, n), check_mask_feather(mask_feather, n)
    seamless = _share(seamless, n, 'seamless', ('[0, 1]', lambda v: (v >= 0.0) & (v <= 1.0),
                                                'the share of the mean-value correction that is added to the donor\'s pixels'))
    ring = check_ring(ring)
    if seamless.any() and mask != 'hull':
        raise ValueError("seamless > 0 needs mask='hull' (the correction is fitted to the outline of the mask), got mask=%r" % (mask,))
    return MorphPlan(photos=photos, rows=rows, donors=donors, donor_rows=full, donor_rows_given=drows, shape=shape, texture=texture,
                     feather=feather, anchors=m, lam=lam, M=M, landmarks=landmarks, donor_landmarks=donor_landmarks, colour=colour,
                     max_gain=max_gain, mask=mask, grow=grow, mask_feather=mask_feather, inv_soft=hull_inv_soft(rows, mask_feather),
                     seamless=seamless, ring=ring)


def colour_moments(sums):
    """imm_colour_stats_u8's sums [n, 7] (read as unsigned) -> (count int64 [n], mean f64 [n, 3], standard deviation f64 [n, 3]) on the
    host, in imm_colour_gain's order of operations: m = S1 / N, sd = sqrt(max(S2 / N - m * m, 0)).  A row without pixels: count 0, NaN."""
    s = np.ascontiguousarray(sums).view(np.uint64) if np.asarray(sums).dtype == np.int64 else np.asarray(sums, dtype=np.uint64)
    N = s[:, 6].astype(np.float64)[:, None]
    with np.errstate(all='ignore'):
        m, q = s[:, 0:3].astype(np.float64) / N, s[:, 3:6].astype(np.float64) / N
        sd = np.sqrt(np.maximum(q - m * m, 0.0))
    return s[:, 6].astype(np.int64), m, sd


class PhotoMorph(object):
    """What morph(return_transform=True) returns: the two splines of every row.  coef_a and coef_b f32 [n, M + 3, 2] (device tensors, the
    halves of imm_warp_fit's output: target frame -> own frame, target frame -> donor frame) on the shared control points ctrl f32
    [n, M, 2]; rows and donor_rows int32 [n, 5] (host); mu and donor_mu f32 [n, K, 2] (the faces' own and the donors' landmarks), poses
    f32 [n, K, 2] (their blend, the target), flags int32 [n] (the OR of the two fits' flags; bit 0: no usable fit, the box was left
    alone), shape and texture f32 [n] (host), and the call's lam and anchors.  With colour matching (morph(colour > 0)): colour f32 [n]
    (host), max_gain, colour_gain f32 [n, 3, 2] (device: (gain, offset) per channel, what the donor's samples were taken through) and
    colour_flags int32 [n] (device; bit 0: a region without pixels, the row got (1, 0)); without it colour_gain and colour_flags are
    None.  With the landmark-hull mask (morph(mask='hull')): mask 'hull', grow, mask_feather and inv_soft f32 [n] (host), hull_edges f32
    [n, K, 3] (device: the lines (ny, nx, d) of every row's grown hull in box-relative pixels, imm_hull_fit's output) and hull_flags
    int32 [n] (device; bit 0: an empty box, a pose or a grow that is not finite; bit 1: no hull with an inside; a flagged row wrote
    nothing; OR-ed into nothing else), and hull_weight(i), the weight over row i's box; without it mask, hull_edges and hull_flags are
    None.  With the membrane (morph(seamless > 0)): seamless f32 [n] (host), ring (the samples per row), seam_ring f32 [n, ring, 2]
    (device: the samples of the mask's outline in box-relative pixels), seam_diff f32 [n, ring, 3] (device: the photo minus the morph's
    mix at every sample), seam_flags int32 [n] (device; bit 0: the hull is flagged or the landmarks' centroid is not strictly inside
    the mask cut with the box; bit 1: a ray without a positive finite length; a flagged row was pasted as the plain hull morph) and
    seam_field(i), the correction over row i's box; without it all of these are None."""

    def __init__(self, coef_a, coef_b, ctrl, rows, donor_rows, mu, donor_mu, poses, flags, shape, texture, lam, anchors, colour=None,
                 max_gain=None, colour_gain=None, colour_flags=None, mask=None, grow=None, mask_feather=None, inv_soft=None,
                 hull_edges=None, hull_flags=None, seamless=None, ring=None, seam_ring=None, seam_diff=None, seam_flags=None):
        self.coef_a, self.coef_b, self.ctrl = coef_a, coef_b, ctrl
        self.rows, self.donor_rows = np.asarray(rows, dtype=np.int32), np.asarray(donor_rows, dtype=np.int32)
        self.mu, self.donor_mu, self.poses, self.flags = mu, donor_mu, poses, flags
        self.shape, self.texture = np.asarray(shape, dtype=np.float32), np.asarray(texture, dtype=np.float32)
        self.lam, self.anchors = float(lam), int(anchors)
        self.colour = np.zeros(len(self.rows), dtype=np.float32) if colour is None else np.asarray(colour, dtype=np.float32)
        self.max_gain = None if max_gain is None else float(max_gain)
        self.colour_gain, self.colour_flags = colour_gain, colour_flags
        self.mask = mask
        self.grow, self.mask_feather, self.inv_soft = (None if a is None else np.asarray(a, dtype=np.float32) for a in (grow, mask_feather, inv_soft))
        self.hull_edges, self.hull_flags = hull_edges, hull_flags
        self.seamless = None if seamless is None else np.asarray(seamless, dtype=np.float32)
        self.ring = None if ring is None else int(ring)
        self.seam_ring, self.seam_diff, self.seam_flags = seam_ring, seam_diff, seam_flags

    def seam_field(self, i):
        """f32 [H_i, W_i, 3]: the correction r at every pixel of row i's box, from the device's seam_ring and seam_diff in the rule's f32
        order (include/imm_seam.h).  The kernel adds seamless[i] * r to the mix of every pixel whose hull weight is > 0."""
        if self.seam_ring is None:
            raise ValueError('seam_field needs a morph with seamless > 0')
        _img, y0, x0, y1, x1 = (int(v) for v in self.rows[i])
        return seam_field(_host(self.seam_ring[i]), _host(self.seam_diff[i]), y1 - y0, x1 - x0)

    def hull_weight(self, i):
        """f32 [H_i, W_i]: the mask's weight at every pixel of row i's box, from the device's hull_edges in the rule's f32 order
        (include/imm_hull.h): dist = min over the slots of (ny * rr + nx * cc) + d at rr = r - y0, cc = c - x0, w = clamp(dist *
        inv_soft, 0, 1).  The kernel blends a pixel with w > 0 by the edge ramp times w and leaves every other alone."""
        if self.hull_edges is None:
            raise ValueError("hull_weight needs a morph with mask='hull'")
        _img, y0, x0, y1, x1 = (int(v) for v in self.rows[i])
        e = np.asarray(_host(self.hull_edges[i]), dtype=np.float32)
        rr, cc = np.arange(max(y1 - y0, 0), dtype=np.float32)[:, None], np.arange(max(x1 - x0, 0), dtype=np.float32)[None, :]
        dist = np.full((rr.shape[0], cc.shape[1]), np.inf, dtype=np.float32)
        with np.errstate(all='ignore'):
            for ny, nx, d in e:
                dist = np.fmin(dist, (ny * rr + nx * cc) + d)
            w = np.fmin(np.fmax(dist * self.inv_soft[i], np.float32(0)), np.float32(1))
        assert w.dtype == np.float32
        return w

    def _frame(self, points_px):
        pts = np.asarray(points_px, dtype=np.float64)
        n = len(self.rows)
        if pts.ndim != 3 or pts.shape[0] != n or pts.shape[2] != 2:
            raise ValueError('points_px must be [%d, P, 2], got %s' % (n, pts.shape))
        org = self.rows[:, 1:3].astype(np.float64)
        half = (self.rows[:, 3:5] - self.rows[:, 1:3]).astype(np.float64) / 2.0
        return pts, org, half

    def to_source(self, points_px):
        """points_px [n, P, 2]: (y, x) photo pixels of the RESULT, row b's in the photo of row b -> f64 [n, P, 2], the pixels of the
        ORIGINAL photo whose values the morph took there (the kernel's map sA, in f64 from the f32 coefficients; blending and clamping
        apart)."""
        pts, org, half = self._frame(points_px)
        coef, ctrl = _host(self.coef_a), _host(self.ctrl)
        out = np.empty_like(pts)
        for b in range(len(self.rows)):
            q = (pts[b] - org[b]) / half[b] - 1.0
            out[b] = pts[b] + half[b] * displacement(coef[b], ctrl[b], q)
        return out

    def to_donor(self, points_px):
        """points_px [n, P, 2] as to_source takes them -> f64 [n, P, 2], the pixels of row b's DONOR photo whose values the morph mixed in
        there (the kernel's map sB: the donor-frame point q + DB(q) in the pixels of the donor box)."""
        pts, org, half = self._frame(points_px)
        coef, ctrl = _host(self.coef_b), _host(self.ctrl)
        dorg = self.donor_rows[:, 1:3].astype(np.float64)
        dhalf = (self.donor_rows[:, 3:5] - self.donor_rows[:, 1:3]).astype(np.float64) / 2.0
        out = np.empty_like(pts)
        for b in range(len(self.rows)):
            q = (pts[b] - org[b]) / half[b] - 1.0
            out[b] = dorg[b] + ((q + displacement(coef[b], ctrl[b], q)) + 1.0) * dhalf[b]
        return out
