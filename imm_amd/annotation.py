"""Annotation: landmarks, boxes, hulls and numbers drawn into u8 photos and clips on the device (include/imm_annotate.h states the rule).

    out = det.annotate(photos, boxes)                                 # every box framed, its landmarks as the project's markers
    out = det.annotate(photos, boxes, draw=('points', 'box', 'hull', 'label'), grow=1.25)
    ca = det.annotate_clip(frames, boxes, trail=8, gate=gate)         # the faces of frames[0] followed; trails; frames coloured by status
    ca.frames[t], ca.track, ca.status                                 # u8 [h_t, w_t, 3], a Track, int32 [T, F]
    ca = det.annotate_clip(frames, track=track)                       # a Track the caller already has, drawn

The instrument for choosing a gate, a grow, a box_smooth or a blocks on one's own footage: what the detector, the tracker, the quality
gate and the hull mask decided, in the same u8 buffers and at the speed the frames are produced.  imm_amd/utils/plot_landmarks.py draws
PIL markers on the host, one enlarged image at a time, and stays as it is; the marker styles here are its table (8 colours x 7 shapes).

The frame of a face takes the colour of its status: STATUS_PALETTE = (ok, lost, outside, unsure), the lowest set bit of the tracker's
flags (bit 0 lost, bit 1 outside) with the gate's verdict OR-ed in as bit 2 (tracking.FLAG_UNSURE).  A lost face draws its
frame and label only: its landmarks are not to be believed.

This module holds the host side: the style tables, plan_annotate (every argument checked before anything reaches the device),
PhotoAnnotation and ClipAnnotation (the results) and run_clip (the launches of annotate_clip).  It imports without a GPU."""
import math

import numpy as np

from . import morphing as MP
from .inference import _Plan
from .tracking import FLAG_LOST, FLAG_OUTSIDE, FLAG_UNSURE        # noqa: F401  the bits of a status
from .utils.plot_landmarks import COLORS, MARKERS

DRAW = ('points', 'box', 'hull', 'label')
BITS = {'points': 1, 'box': 2, 'hull': 4, 'label': 8}            # IMM_ANNOTATE_*
MAX_GROUPS, MAX_PAD, MAX_K = 16, 64, 80
# ok, lost, outside, unsure: the frame of a row takes palette[0] for status 0, else palette[1 + its lowest set bit]
STATUS_PALETTE = np.array([(40, 220, 60), (235, 30, 30), (255, 150, 0), (250, 230, 20)], dtype=np.uint8)
# seven rows of five columns per digit, as include/imm_annotate.h prints them in hex
FONT = np.array([[0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E], [0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E], [0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F],
                 [0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E], [0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02], [0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E],
                 [0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E], [0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08], [0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E],
                 [0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C]], dtype=np.uint8)


def mark_styles(K):
    """u8 [K, 4]: (r, g, b, shape) of landmark k, plot_landmarks.get_marker_style's table: colour cycles fastest, the shape (its index in
    plot_landmarks.MARKERS) changes every 8 landmarks.  Past its 56 styles the table starts again (get_marker_style raises there)."""
    n = len(COLORS) * len(MARKERS)
    return np.array([tuple(COLORS[(k % n) % len(COLORS)]) + ((k % n) // len(COLORS),) for k in range(int(K))], dtype=np.uint8).reshape(-1, 4)


def group_styles(size, groups, alpha):
    """f32 [G, 4]: (R, 1 / (2 R), h, alpha) per group.  The last group holds the markers: R = size, half stroke h = max(0.5, size / 4).
    The groups before it are the trail, oldest first: discs of radius max(0.5, size / 2) whose alpha rises from alpha * 0.7 / G."""
    G, size, alpha = int(groups), float(size), float(alpha)
    out = np.empty((G, 4), dtype=np.float64)
    for g in range(G):
        last = g == G - 1
        R = size if last else max(0.5, 0.5 * size)
        out[g] = (R, 1.0 / (2.0 * R), max(0.5, 0.25 * size), alpha if last else alpha * 0.7 * (g + 1) / G)
    return out.astype(np.float32)


def draw_bits(draw):
    if isinstance(draw, str):
        draw = tuple(d for d in draw.split(',') if d)
    if not isinstance(draw, (list, tuple)) or any(not isinstance(d, str) or d not in BITS for d in draw):
        raise ValueError("draw must be a subset of ('points', 'box', 'hull', 'label'), got %r" % (draw,))
    return sum(BITS[d] for d in set(draw))


def default_pad(size):
    return int(math.ceil(float(size))) + 2


def grid_pixels(rows, pad):
    """max_box_pixels of an annotate launch: the pixels of the largest extent (a box grown by pad on every side).  It sizes the grid
    only."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    side = np.maximum(rows[:, 3:5] - rows[:, 1:3], 0) + 2 * int(pad)
    return int(max(1, min(int((side[:, 0] * side[:, 1]).max()), 2 ** 31 - 1)))


def _number(name, v, lo, hi, open_lo=False):
    try:
        f = float(v)
    except (TypeError, ValueError):
        f = float('nan')
    if isinstance(v, bool) or not ((lo < f if open_lo else lo <= f) and f <= hi):
        raise ValueError('%s must lie in %s%g, %g], got %r' % (name, '(' if open_lo else '[', lo, hi, v))
    return f


def _integer(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError('%s must be an int in [%d, %d], got %r' % (name, lo, hi, v))
    return int(v)


def check_style(K, draw, size, thickness, trail, alpha, pad, label_scale):
    """The settings every annotate call shares -> (bits, size, thickness, trail, alpha, pad, label_scale); a ValueError names the first
    that is out of range."""
    bits = draw_bits(draw)
    if not 1 <= int(K) <= MAX_K:
        raise ValueError('annotation serves 1..%d landmarks, got K = %r' % (MAX_K, K))
    size = _number('size', size, 0.0, 32.0, open_lo=True)
    thickness = _integer('thickness', thickness, 1, 16)
    trail = _integer('trail', trail, 0, MAX_GROUPS - 1)
    alpha = _number('alpha', alpha, 0.0, 1.0, open_lo=True)
    pad = default_pad(size) if pad is None else _integer('pad', pad, 0, MAX_PAD)
    return bits, size, thickness, trail, alpha, pad, _integer('label_scale', label_scale, 1, 8)


def check_row_ints(name, v, shape):
    """labels / status: None or integers of `shape` -> int32 array."""
    if v is None:
        return None
    a = np.asarray(v.cpu() if hasattr(v, 'cpu') else v)
    if a.shape != tuple(shape) or a.dtype.kind not in 'iu':
        raise ValueError('%s must be integers of shape %s, got %s %s' % (name, tuple(shape), a.dtype, a.shape))
    return np.ascontiguousarray(a, dtype=np.int32)


class AnnotatePlan(_Plan):
    """What plan_annotate returns, by name: photos (decoded u8 arrays), rows int32 [n, 5], bits (draw as IMM_ANNOTATE_* bits), size,
    thickness, trail, alpha, pad, label_scale, labels int32 [n] or None, status int32 [n] or None, grow f32 [n], landmarks (None or an f32
    tensor [n, K, 2]), mark_style u8 [K, 4], group_style f32 [trail + 1, 4], palette u8 [4, 3], max_pixels (grid_pixels of the rows)."""
    FIELDS = ('photos', 'rows', 'bits', 'size', 'thickness', 'trail', 'alpha', 'pad', 'label_scale', 'labels', 'status', 'grow', 'landmarks',
              'mark_style', 'group_style', 'palette', 'max_pixels')


def plan_annotate(photos, boxes, K, landmarks=None, draw=('points', 'box'), size=2.5, thickness=1, labels=None, status=None, grow=1.25,
                  alpha=1.0, trail=0, pad=None, label_scale=1):
    """annotate()'s arguments checked on the host, before anything reaches the device: an AnnotatePlan.  photos / boxes in
    generation.plan_repose's forms (a list of u8 arrays; box rows, by default one whole-photo box per photo).  draw: a subset of
    ('points', 'box', 'hull', 'label'); size in (0, 32] (the markers' radius in pixels); thickness an int in [1, 16]; trail an int in
    [0, 15]; alpha in (0, 1]; pad an int in [0, 64], by default ceil(size) + 2; label_scale an int in [1, 8]; labels and status None or
    integers [n] (labels=None with 'label' numbers the rows); grow as morph takes it; landmarks None or [n, K, 2] in the frame of the
    boxes (redact's convention; values that are not finite are not refused: they draw nothing); at most 65535 rows."""
    from .generation import NEEDS_U8
    from .inference import check_landmarks, photos_and_rows
    bits, size, thickness, trail, alpha, pad, label_scale = check_style(K, draw, size, thickness, trail, alpha, pad, label_scale)
    needs = 'photos: %s' % NEEDS_U8
    photos, rows = photos_and_rows(photos, boxes, needs, needs,
                                   limit=(65535, 'an annotation serves at most 65535 rows a call (n <= 65535), got n = %d'))
    n = len(rows)
    labels, status = check_row_ints('labels', labels, (n,)), check_row_ints('status', status, (n,))
    if labels is None and bits & BITS['label']:
        labels = np.arange(n, dtype=np.int32)
    grow = MP.check_grow(grow, n)
    if landmarks is not None:
        landmarks = check_landmarks(landmarks, (n,), K)
    return AnnotatePlan(photos=photos, rows=rows, bits=bits, size=size, thickness=thickness, trail=trail, alpha=alpha, pad=pad,
                        label_scale=label_scale, labels=labels, status=status, grow=grow, landmarks=landmarks, mark_style=mark_styles(K),
                        group_style=group_styles(size, trail + 1, alpha), palette=STATUS_PALETTE.copy(), max_pixels=grid_pixels(rows, pad))


class PhotoAnnotation(object):
    """What annotate(return_transform=True) returns.  rows int32 [n, 5] (host); points f32 [n, K, 2] (device: the landmarks in photo
    pixels, imm_annotate_points' output: where the markers were drawn); hull_edges f32 [n, K, 3] and hull_flags int32 [n] (device:
    imm_hull_fit's output) when the hull was drawn, else None; status int32 [n] (host) or None."""

    def __init__(self, rows, points, hull_edges=None, hull_flags=None, status=None):
        self.rows, self.points, self.hull_edges, self.hull_flags, self.status = np.asarray(rows, dtype=np.int32), points, hull_edges, hull_flags, status


class ClipAnnotation(object):
    """What annotate_clip returns, T frames by F faces: frames: frames[t] is frame t drawn into, u8 [h_t, w_t, 3] on the detector's
    device, views of one packed canvas per chunk; track: the tracking.Track of the faces (the caller's own with track=); status int32
    [T, F] on the device: the tracker's flags (bit 0 lost, bit 1 outside) with the gate's verdict as bit 2 (FLAG_UNSURE)."""

    def __init__(self, frames, track, status):
        self.frames, self.track, self.status = frames, track, status

    def __len__(self):
        return len(self.frames)


class ClipAnnotatePlan(_Plan):
    """annotate_clip()'s checked arguments: frames (decoded u8 arrays), rows int32 [F, 5] (with boxes) or None, track (with track=) or
    None, style (the AnnotatePlan of the first frame's rows: every setting of the drawing), smooth, box_smooth, one_euro, fps,
    chunk_frames, gate."""
    FIELDS = ('frames', 'rows', 'track', 'style', 'smooth', 'box_smooth', 'one_euro', 'fps', 'chunk_frames', 'gate')


def plan_annotate_clip(frames, boxes, track, K, draw=('points', 'box'), trail=0, smooth=True, gate=None, size=2.5, thickness=1, labels=None,
                       grow=1.25, alpha=1.0, pad=None, label_scale=1, box_smooth=0.5, one_euro=None, fps=25.0, chunk_frames=32,
                       max_batch=256):
    """annotate_clip()'s arguments checked on the host, before anything reaches the device: a ClipAnnotatePlan.  Exactly one of boxes
    (the faces of frames[0]: tracking.plan_track's checks) and track (a tracking.Track of these frames) is given."""
    from . import tracking as TR
    if (boxes is None) == (track is None):
        raise ValueError('annotate_clip takes exactly one of boxes (the faces of the first frame) and track (a Track to draw)')
    if track is None:
        frames, rows, beta, _consts, chunk = TR.plan_track(frames, boxes, max_batch, box_smooth, one_euro, fps, chunk_frames, gate)
    else:
        if not isinstance(track, TR.Track):
            raise ValueError('track must be a tracking.Track, got %r' % (type(track).__name__,))
        T, F = int(track.boxes.shape[0]), int(track.boxes.shape[1])
        if tuple(track.points.shape) != (T, F, int(K), 2):
            raise ValueError('track.points must be [%d, %d, %d, 2], got %s' % (T, F, int(K), tuple(track.points.shape)))
        first = np.asarray(track.boxes[0].cpu() if hasattr(track.boxes, 'cpu') else track.boxes[0]).reshape(F, 4)
        frames, rows, beta, _consts, chunk = TR.plan_track(frames, first.tolist(), max(F, 1), chunk_frames=chunk_frames)
        if len(frames) != T:
            raise ValueError('the track holds %d frames, %d were given' % (T, len(frames)))
    style = plan_annotate(frames[:1], rows.tolist(), K, None, draw, size, thickness, labels, None, grow, alpha, trail, pad, label_scale)
    return ClipAnnotatePlan(frames=frames, rows=rows, track=track, style=style, smooth=bool(smooth), box_smooth=beta, one_euro=one_euro,
                            fps=float(fps), chunk_frames=chunk, gate=gate)


def run_clip(det, plan):
    """The launches of annotate_clip() for a checked plan; called with the caller's stream current.  The frame loop is
    tracking.run_frames: per chunk one upload and one canvas copy; per frame, on the detector's stream, FaceTracker._advance (skipped
    with track=), imm_hull_fit on the frame's landmarks (Track.mu) when the hull is drawn and ONE imm_annotate_u8 launch whose marks
    are a view of the slots [t - trail', t] of the tracker's points (points_smooth with smooth=True), trail' = min(trail, t): the start
    of a clip uses fewer groups, never another clip's data.  The status is formed on the device: the tracker's flags with the gate's
    verdict OR-ed in as bit 2.  Nothing returns to the host between the first and the last frame's launches."""
    import torch
    from . import ops
    from . import tracking as TR
    from .clip import GRID_AREAS
    from .generation import compose_links
    from .inference import _Held
    st, frames, rows, track = plan.style, plan.frames, plan.rows, plan.track
    K, dev = det.K, det.dev
    F, T, bits = len(rows), len(frames), st.bits
    hull, points = bool(bits & BITS['hull']), bool(bits & BITS['points'])
    max_pixels = int(min(GRID_AREAS * st.max_pixels, 2 ** 31 - 1))
    held = _Held(dev)                                          # what the loop's _join records: every tensor made below
    up = held.up
    with torch.cuda.device(dev):
        links_d, palette_d, mstyle_d = up(compose_links(rows)), up(st.palette), up(st.mark_style)
        # group_style of every G the clip uses: the first frames have fewer groups than trail + 1
        gstyles = [up(group_styles(st.size, G, st.alpha)) for G in range(1, min(st.trail, T - 1) + 2)]
        labels_d = None if st.labels is None else up(st.labels)
        grow_d = edges = hflags = None
        if hull:
            grow_d = up(st.grow)
            edges, hflags = held.empty(F, K, 3), held.empty(F, dtype=torch.int32)
        if track is None:
            tracker = TR.FaceTracker(det, None, plan.box_smooth, plan.one_euro, plan.fps, capacity=T, gate=plan.gate)
            status = held.empty(T, F, dtype=torch.int32)
        else:
            # the Track's tensors on the device, as the tracker's buffers hold them; the rows of frame t name its place in its chunk
            tracker = None
            on = lambda t: torch.as_tensor(t).to(device=dev).contiguous()
            t_mu, t_flags = held.keep(on(track.mu).float(), on(track.flags).int())
            t_pts = held.keep(on(track.points_smooth if plan.smooth else track.points).float())
            t_rows = held.zeros(T, F, 5, dtype=torch.int32)
            t_rows[:, :, 1:] = on(track.boxes).int()
            t_rows[:, :, 0] = (torch.arange(T, device=dev, dtype=torch.int32) % plan.chunk_frames)[:, None]
            status = held.keep(t_flags.clone())
            if track.qflags is not None:
                TR.or_unsure(status, on(track.qflags))

    def frame(t, f):
        if track is None:
            b = f.bufs
            rows_t, mu_t, pts = b['boxes'][t], b['mu'][t], b['smooth' if plan.smooth else 'points']
            status[t].copy_(b['flags'][t])
            if plan.gate is not None:
                TR.or_unsure(status[t], b['qflags'][t])
        else:
            rows_t, mu_t, pts = t_rows[t], t_mu[t], t_pts
        G = min(st.trail, t) + 1
        extra = {}
        if hull:
            ops.hull_fit(mu_t, rows_t, grow_d, edges, hflags)
            extra['edges'] = edges
        if points:
            extra.update(marks=pts[t + 1 - G:t + 1], group_style=gstyles[G - 1], mark_style=mstyle_d)
        ops.annotate_u8(f.canvas, f.offs, f.hw, rows_t, links_d, palette_d, bits, st.thickness, st.pad, st.label_scale, max_pixels,
                        status=status[t], labels=labels_d, **extra)

    out = TR.run_frames(det, frames, plan.chunk_frames, held, frame, tracker, rows)
    return ClipAnnotation(out, tracker.result() if track is None else track, status)
