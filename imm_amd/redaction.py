"""Redaction: faces pixelated or smoothed inside their u8 photos and clips (include/imm_redact.h states the rule).

    out = det.redact(photos, boxes)                        # the photos with every box a mosaic of 8 cells along its longer side
    out = det.redact(photos, boxes, mode='smooth', mask='hull')          # a blur, over the landmark hull only
    cr = det.redact_clip(frames, boxes)                    # the faces of frames[0] followed and redacted on every frame
    cr.frames[t], cr.track, cr.own, cr.hull_flags          # u8 [h_t, w_t, 3], a Track, f32 [T, F, K, 2], int32 [T, F] or None

repose, warp, morph, morph_clip and reenact turn a face into another face; this is the opposite operation.  The box of a face is cut
into square cells of side ceil(max(H, W) / blocks); every cell takes the mean of the ORIGINAL pixels it covers (imm_redact_cells_u8, in
integers), and the box is pasted over with those means ('pixelate') or with their bilinear interpolation ('smooth'), through the
skeleton of the other paste kernels (imm_redact_u8).  The cells are anchored to the box, so the mosaic travels with a tracked face.

Redaction FAILS CLOSED.  morph leaves a row alone whose hull is degenerate, whose landmarks are not finite or whose track is lost; here
such a row is redacted over its whole box: with mask='hull' imm_hull_fit flags it and the paste gives it the weight 1 everywhere, and
without a mask the whole box is covered anyway.  A face the tracker lost on a frame keeps the box the tracker's unchanged state gives
it, and that box is covered: a lost face is never shown.  The tracker never loses a face on the FIRST frame (the caller vouches for
the first boxes), so with a gate redact_clip folds the gate's verdict into the flags itself: a face the gate finds unsure on any frame,
the first included, is covered whole.  The defaults blocks=8, feather=0 and mask=None are the conservative reading
(the hard, whole box).  Nobody has measured how recognisable a face stays at any setting: this module ships no claim of anonymity.

redact_clip follows only the faces boxed on the first frame.  A face that enters the clip later is NOT redacted: detection of new
faces is out of scope.

This module holds the host side: the cell arithmetic, plan_redact (every argument checked before anything reaches the device),
PhotoRedaction and ClipRedaction (the results) and run_clip (the launches of redact_clip).  It imports without a GPU."""
import numpy as np

from . import morphing as MP
from .inference import _Plan
from .tracking import FLAG_UNSURE              # noqa: F401  ClipRedaction.hull_flags: bit 2, the gate found the face unsure on that frame
from .warping import _host

MODES = {'pixelate': 0, 'smooth': 1}      # IMM_REDACT_PIXELATE, IMM_REDACT_SMOOTH
MAX_BLOCKS = 64                           # cells along the longer side of a box


def cell_size(H, W, blocks):
    """The side of the square cells of an H x W box: max(1, ceil(max(H, W) / blocks)), in integers; 0 for an empty box."""
    H, W, blocks = int(H), int(W), int(blocks)
    if H <= 0 or W <= 0:
        return 0
    return max(1, (max(H, W) + blocks - 1) // blocks)


def grid_shape(H, W, blocks):
    """(gy, gx): the cells along each side of an H x W box, both <= blocks; (0, 0) for an empty box."""
    cell = cell_size(H, W, blocks)
    if not cell:
        return 0, 0
    return (int(H) + cell - 1) // cell, (int(W) + cell - 1) // cell


def check_mode(mode):
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError("mode must be 'pixelate' or 'smooth', got %r" % (mode,))
    return mode


def check_blocks(blocks):
    if isinstance(blocks, bool) or not isinstance(blocks, (int, np.integer)) or not 1 <= int(blocks) <= MAX_BLOCKS:
        raise ValueError('blocks must be an int in [1, %d] (the cells along the longer side of a box), got %r' % (MAX_BLOCKS, blocks))
    return int(blocks)


class RedactPlan(_Plan):
    """What plan_redact returns, by name: photos (decoded u8 arrays), rows int32 [n, 5], mode ('pixelate' or 'smooth'), blocks, feather,
    mask (None or 'hull'), grow f32 [n], mask_feather f32 [n], inv_soft f32 [n] (morphing.hull_inv_soft of the rows) and landmarks (None
    or an f32 tensor [n, K, 2]; it may hold values that are not finite: such a row is redacted whole)."""
    FIELDS = ('photos', 'rows', 'mode', 'blocks', 'feather', 'mask', 'grow', 'mask_feather', 'inv_soft', 'landmarks')


def plan_redact(photos, boxes, K, mode='pixelate', blocks=8, mask=None, grow=1.25, mask_feather=0.1, feather=0.0, landmarks=None):
    """redact()'s arguments checked on the host, before anything reaches the device: a RedactPlan.  photos / boxes in
    generation.plan_repose's forms (a list of u8 arrays; box rows, by default one whole-photo box per photo).  mode: 'pixelate' or
    'smooth'; blocks: an int in [1, 64]; feather in [0, 0.5]; mask: None or 'hull'; grow and mask_feather as morph takes them (checked
    whatever mask is).  landmarks: None or [n, K, 2]; values that are not finite are NOT refused: redaction fails closed, and such a
    row is redacted over its whole box."""
    from .generation import NEEDS_U8, check_feather
    from .inference import check_landmarks, photos_and_rows
    mode, blocks = check_mode(mode), check_blocks(blocks)
    if mask not in MP.MASKS:
        raise ValueError("mask must be None or 'hull', got %r" % (mask,))
    feather = check_feather(feather)
    needs = 'photos: %s' % NEEDS_U8
    photos, rows = photos_and_rows(photos, boxes, needs, needs, limit=(65535, 'a redaction serves at most 65535 rows a call, got %d'))
    n = len(rows)
    grow, mask_feather = MP.check_grow(grow, n), MP.check_mask_feather(mask_feather, n)
    if landmarks is not None:
        landmarks = check_landmarks(landmarks, (n,), K)
    return RedactPlan(photos=photos, rows=rows, mode=mode, blocks=blocks, feather=feather, mask=mask, grow=grow, mask_feather=mask_feather,
                      inv_soft=MP.hull_inv_soft(rows, mask_feather), landmarks=landmarks)


class PhotoRedaction(object):
    """What redact(return_transform=True) returns.  rows int32 [n, 5] (host); cells u8 [n, blocks * blocks * 3] (device: every row's
    grid of means, dense as [gy, gx, 3] at the start of its slice, imm_redact_cells_u8's output); cell int64 [n] and grid int64 [n, 2]
    (host: every row's cell side and (gy, gx)); mode and blocks (the call's); and with mask='hull': mu f32 [n, K, 2] (device: the
    landmarks the hull was fitted to), hull_edges f32 [n, K, 3] and hull_flags int32 [n] (device: imm_hull_fit's output; a row whose
    flag is not 0 was redacted over its WHOLE box), inv_soft f32 [n] (host); without the mask these four are None.  weight(i) is the
    weight map of row i."""

    def __init__(self, rows, cells, mode, blocks, feather, mu=None, hull_edges=None, hull_flags=None, inv_soft=None):
        self.rows, self.cells, self.mode, self.blocks, self.feather = np.asarray(rows, dtype=np.int32), cells, mode, int(blocks), float(feather)
        hw = self.rows[:, 3:5].astype(np.int64) - self.rows[:, 1:3]
        self.cell = np.array([cell_size(h, w, blocks) for h, w in hw], dtype=np.int64)
        self.grid = np.array([grid_shape(h, w, blocks) for h, w in hw], dtype=np.int64).reshape(-1, 2)
        self.mu, self.hull_edges, self.hull_flags = mu, hull_edges, hull_flags
        self.inv_soft = None if inv_soft is None else np.asarray(inv_soft, dtype=np.float32)

    def means(self, i):
        """u8 [gy, gx, 3]: the grid of means of row i, on the host."""
        gy, gx = (int(v) for v in self.grid[i])
        return np.asarray(_host(self.cells[i]))[:gy * gx * 3].reshape(gy, gx, 3)

    def weight(self, i):
        """f32 [H_i, W_i]: the blend weight at every pixel of row i's box, on host arrays in the rule's f32 order
        (include/imm_redact.h): the edge ramp, times the hull's weight with the mask (1 everywhere for a flagged row; 0 where the hull's
        weight is not > 0: the pixel was left alone)."""
        from .generation import compose_inv_ramp
        f32 = np.float32
        _img, y0, x0, y1, x1 = (int(v) for v in self.rows[i])
        H, W = max(y1 - y0, 0), max(x1 - x0, 0)
        iry, irx = compose_inv_ramp(self.rows[i:i + 1], self.feather)[0]
        r, c = np.arange(H), np.arange(W)
        wy = np.minimum(f32(1), (np.minimum(r, H - 1 - r).astype(f32) + f32(0.5)) * iry)
        wx = np.minimum(f32(1), (np.minimum(c, W - 1 - c).astype(f32) + f32(0.5)) * irx)
        a = wy[:, None] * wx[None, :]
        if self.hull_edges is None or int(_host(self.hull_flags[i])) != 0:
            return a
        e = np.asarray(_host(self.hull_edges[i]), dtype=f32)
        rr, cc = np.arange(H, dtype=f32)[:, None], np.arange(W, dtype=f32)[None, :]
        dist = np.full((H, W), np.inf, dtype=f32)
        with np.errstate(all='ignore'):
            for ny, nx, d in e:
                dist = np.fmin(dist, (ny * rr + nx * cc) + d)
            w = np.fmin(np.fmax(dist * self.inv_soft[i], f32(0)), f32(1))
        out = np.where(w > 0, a * w, f32(0))
        assert out.dtype == f32
        return out


class ClipRedaction(object):
    """What redact_clip returns, T frames by F faces, tensors on the detector's device: frames: frames[t] is frame t with its faces
    redacted, u8 [h_t, w_t, 3], views of one packed canvas per chunk; track: the tracking.Track of the faces; own f32 [T, F, K, 2]: the
    landmarks of every frame in the frame of its box (NaN for a face the tracker lost on that frame, or that the gate found unsure:
    its whole box was redacted); hull_flags int32 [T, F] with mask='hull' (bits 0 and 1: imm_hull_fit's flags; bit 2, FLAG_UNSURE: the
    gate found the face unsure on that frame, the first frame included; not 0: the whole box was redacted), else None."""

    def __init__(self, frames, track, own, hull_flags=None):
        self.frames, self.track, self.own, self.hull_flags = frames, track, own, hull_flags

    def __len__(self):
        return int(self.own.shape[0])


class ClipRedactPlan(_Plan):
    """redact_clip()'s checked arguments: frames (decoded u8 arrays), rows int32 [F, 5], redact (the RedactPlan of the first frame's rows:
    every setting of the redaction), smooth, box_smooth, one_euro, fps, chunk_frames, gate."""
    FIELDS = ('frames', 'rows', 'redact', 'smooth', 'box_smooth', 'one_euro', 'fps', 'chunk_frames', 'gate')


def plan_redact_clip(frames, boxes, K, mode='pixelate', blocks=8, mask=None, grow=1.25, mask_feather=0.1, feather=0.0, smooth=True,
                     box_smooth=0.5, one_euro=None, fps=25.0, chunk_frames=32, max_batch=256, gate=None):
    """redact_clip()'s arguments checked on the host, before anything reaches the device: a ClipRedactPlan.  frames, boxes, box_smooth,
    one_euro, fps, chunk_frames and gate go through tracking.plan_track, the redaction's settings through plan_redact with the first
    frame as the one photo."""
    from . import tracking as TR
    frames, rows, beta, _consts, chunk = TR.plan_track(frames, boxes, max_batch, box_smooth, one_euro, fps, chunk_frames, gate)
    redact = plan_redact(frames[:1], rows.tolist(), K, mode, blocks, mask, grow, mask_feather, feather)
    return ClipRedactPlan(frames=frames, rows=rows, redact=redact, smooth=bool(smooth), box_smooth=beta, one_euro=one_euro, fps=float(fps),
                          chunk_frames=chunk, gate=gate)


def run_clip(det, plan):
    """The launches of redact_clip() for a checked plan; called with the caller's stream current.  The frame loop is
    tracking.run_frames: per chunk one upload and one canvas copy; per frame, on the detector's stream, FaceTracker._advance,
    imm_clip_rows, with the mask imm_hull_fit on own[t], imm_redact_cells_u8 from the frame's ORIGINAL pixels and imm_redact_u8 into the
    canvas, with the frame's rows as they lie in the tracker's buffer.  Nothing returns to the host between the first and the last
    frame's launches."""
    import torch
    from . import ops
    from . import tracking as TR
    from .clip import grid_pixels
    from .generation import compose_links
    from .inference import _Held
    rp, frames, rows = plan.redact, plan.frames, plan.rows
    S, K, dev = det.S, det.K, det.dev
    F, T, hull, mode = len(rows), len(frames), rp.mask == 'hull', MODES[rp.mode]
    max_pixels = grid_pixels(rows)
    held = _Held(dev)                                          # what the loop's _join records: every tensor made below
    up, empty = held.up, held.empty
    with torch.cuda.device(dev):
        links_d = up(compose_links(rows))          # all F rows of a frame lie in one photo: these links serve every frame
        own, inv_ramp = empty(T, F, K, 2), empty(T, F, 2)
        cells = empty(F, rp.blocks * rp.blocks * 3, dtype=torch.uint8)
        grow_d = feather_d = inv_soft = edges = hflags = None
        if hull:
            grow_d, feather_d = up(rp.grow), up(rp.mask_feather)
            inv_soft, edges, hflags = empty(T, F), empty(F, K, 3), empty(T, F, dtype=torch.int32)

    def frame(t, f):
        b = f.bufs
        rows_t = b['boxes'][t]
        ops.clip_rows(rows_t, b['flags'][t], b['mu'][t], b['smooth'][t] if plan.smooth else None, S, rp.feather, feather_d, own[t],
                      inv_ramp[t], inv_soft[t] if hull else None)
        extra = {}
        if hull:                                               # a lost face has NaN landmarks: flagged, and redacted whole
            ops.hull_fit(own[t], rows_t, grow_d, edges, hflags[t])
            if plan.gate is not None:
                # the gate's verdict goes into the flag the paste reads: the tracker scores the first frame without losing
                # its faces (the caller vouches for the first boxes), and a face that is unsure there has finite landmarks
                TR.or_unsure(hflags[t], b['qflags'][t])
            extra = dict(edges=edges, inv_soft=inv_soft[t], hull_flags=hflags[t])
        ops.redact_cells_u8(f.src, f.offs, f.hw, rows_t, rp.blocks, cells)
        ops.redact_u8(f.canvas, f.offs, f.hw, rows_t, links_d, inv_ramp[t], cells, rp.blocks, mode, max_pixels, **extra)

    tracker = TR.FaceTracker(det, None, plan.box_smooth, plan.one_euro, plan.fps, capacity=T, gate=plan.gate)
    out = TR.run_frames(det, frames, plan.chunk_frames, held, frame, tracker, rows)
    return ClipRedaction(out, tracker.result(), own, hflags)
