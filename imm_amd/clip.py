"""Clip morph: a donor's face follows a tracked face through a clip, from the pixels of the two photographs.

    cm = det.morph_clip(frames, boxes, donors)             # frames: T u8 arrays, boxes: the F faces of frames[0]; donors: u8 arrays
    cm.frames[t]                                           # frame t with the donors' faces in place, u8 [h_t, w_t, 3]
    cm.track, cm.own, cm.fit_flags                         # a Track, f32 [T, F, K, 2], int32 [T, F]
    cm.colour_gain, cm.seam_diff, ...                      # what was pasted, after the filter; None when that part is off

detector.track follows the faces of a clip and detector.morph blends a donor's face into a photo; this joins the two the way
reenact.py joins the tracker to the generator.  Once per call the donors are packed and uploaded, their landmarks detected (unless
given), their colour sums taken (imm_colour_stats_u8), the links of the paste formed (all F rows of a frame lie in one photo, so
generation.compose_links of the first rows serves every frame) and the per-face settings uploaded.  Per chunk the tracker uploads
the frames and the canvas is a device copy of them: the frame loop is tracking.run_frames.  Per frame, on the detector's stream,
without anything returning to the host between the clip's first and last launch:

    FaceTracker._advance             crop, pose program, imm_track_step, copy: the next frame's box rows stay on the device
    imm_clip_rows                    this frame's rows -> own[t] (the landmarks that are blended), inv_ramp[t], inv_soft[t]
    with colour                      imm_colour_stats_u8 over this frame's rows, imm_colour_gain against the donors' sums;
                                     with colour_smooth < 1 imm_clip_ema filters the gain
    imm_morph_poses, with the mask imm_hull_fit, ONE imm_warp_fit over 2 F rows
    with the membrane                imm_seam_fit; with seam_smooth < 1 imm_clip_ema filters the differences
    ops.morph_paste                  into the chunk's canvas, with the frame's rows as they lie in the tracker's buffer

include/imm_clip.h states the rule of the two kernels that are new here.  A face the tracker lost on a frame gets NaN landmarks from
imm_clip_rows, and the chain documents the rest: imm_morph_poses carries the NaN, imm_warp_fit flags the row and gives it NaN
coefficients, the paste writes nothing there, imm_hull_fit and imm_seam_fit flag it.  The frame keeps its pixels.

colour_smooth and seam_smooth follow the tracker's box_smooth convention, s <- s + a (x - s); 1 means no filter (the launch is not
issued).  Their defaults of 0.25 are by analogy with box_smooth: nobody has tuned them on footage.

This module holds the host side: plan_clip (every argument checked before anything reaches the device), ClipMorph (the result) and
run (the launches).  It imports without a GPU."""
import math

import numpy as np
import torch

from . import morphing as MP
from . import tracking as TR
from .inference import _Plan

GRID_AREAS = 4                 # the paste and stats grids are sized for this many times the first frame's largest box


def check_smooth(value, name):
    """colour_smooth / seam_smooth: a number in (0, 1] -> float."""
    try:
        a = float(value)
    except (TypeError, ValueError):
        raise ValueError('%s must be a number in (0, 1], got %r' % (name, value))
    if not (math.isfinite(a) and 0.0 < a <= 1.0):
        raise ValueError('%s must lie in (0, 1] (the weight of a frame\'s value in the filter; 1: no filter), got %r' % (name, value))
    return a


class ClipPlan(_Plan):
    """morph_clip()'s checked arguments: frames (decoded u8 arrays), rows int32 [F, 5], morph (the morphing.MorphPlan of the first
    frame's rows and the donors: every setting of the morph), smooth, colour_smooth, seam_smooth, box_smooth, one_euro, fps,
    chunk_frames, gate (a quality.QualityGate handed to the tracker, or None)."""
    FIELDS = ('frames', 'rows', 'morph', 'smooth', 'colour_smooth', 'seam_smooth', 'box_smooth', 'one_euro', 'fps', 'chunk_frames', 'gate')


def plan_clip(frames, boxes, donors, donor_boxes=None, shape=0.0, texture=1.0, feather=0.125, K=10, anchors=2, lam=0.0,
              donor_landmarks=None, colour=0.0, max_gain=2.0, mask=None, grow=1.25, mask_feather=0.1, seamless=0.0, ring=128, smooth=True,
              colour_smooth=0.25, seam_smooth=0.25, box_smooth=0.5, one_euro=TR.OneEuro(), fps=25.0, chunk_frames=32, max_batch=256,
              gate=None):
    """morph_clip()'s arguments checked on the host, before anything reaches the device: a ClipPlan.  frames, boxes, box_smooth, one_euro,
    fps and chunk_frames go through tracking.plan_track, the donors and the morph's settings through morphing.plan_morph with the first
    frame as the one photo (its checks and refusals are the morph's own); colour_smooth and seam_smooth must lie in (0, 1]."""
    colour_smooth, seam_smooth = check_smooth(colour_smooth, 'colour_smooth'), check_smooth(seam_smooth, 'seam_smooth')
    frames, rows, beta, _consts, chunk = TR.plan_track(frames, boxes, max_batch, box_smooth, one_euro, fps, chunk_frames, gate)
    morph = MP.plan_morph(frames[:1], donors, rows.tolist(), donor_boxes, shape, texture, feather, K, anchors, lam, None, donor_landmarks,
                          colour, max_gain, mask, grow, mask_feather, seamless, ring)
    return ClipPlan(frames=frames, rows=rows, morph=morph, smooth=bool(smooth), colour_smooth=colour_smooth, seam_smooth=seam_smooth,
                    box_smooth=beta, one_euro=one_euro, fps=float(fps), chunk_frames=chunk, gate=gate)


class ClipMorph(object):
    """What morph_clip returns, T frames by F faces, tensors on the detector's device:
    frames: frames[t] is frame t with the donors' faces in place, u8 [h_t, w_t, 3], views of one packed canvas per chunk; track: the
    tracking.Track of the faces; own f32 [T, F, K, 2]: the landmarks that were blended ((y, x) in [-1, 1] of each frame's box; NaN for a
    face the tracker lost on that frame, which was not pasted); fit_flags int32 [T, F] (the OR of the two fits' flags; bit 0: no usable
    fit, the box was left alone).  With colour matching: colour_gain f32 [T, F, 3, 2] ((gain, offset) per channel, the values pasted,
    after the filter) and colour_flags int32 [T, F]; with the mask: hull_flags int32 [T, F]; with the membrane: seam_diff f32
    [T, F, ring, 3] (the values pasted, after the filter) and seam_flags int32 [T, F]; each is None when that part is off."""

    def __init__(self, frames, track, own, fit_flags, colour_gain=None, colour_flags=None, hull_flags=None, seam_diff=None, seam_flags=None):
        self.frames, self.track, self.own, self.fit_flags = frames, track, own, fit_flags
        self.colour_gain, self.colour_flags, self.hull_flags = colour_gain, colour_flags, hull_flags
        self.seam_diff, self.seam_flags = seam_diff, seam_flags

    def __len__(self):
        return int(self.own.shape[0])


def grid_pixels(rows):
    """max_box_pixels of the stats and paste launches of every frame: GRID_AREAS times the area of the first frame's largest box.  It
    sizes grids only: the kernels walk a larger box with the same grid."""
    from .generation import box_areas
    return int(max(1, min(GRID_AREAS * int(box_areas(np.asarray(rows)).max()), 2 ** 31 - 1)))


def run(det, plan):
    """The launches of morph_clip() for a checked plan (see the module docstring); called with the caller's stream current.  The frame
    loop is tracking.run_frames; `frame` is what a frame adds behind the tracker's launches."""
    from . import ops
    from . import warping as WP
    from .generation import box_areas, compose_links
    from .inference import _Held, pack_u8, pose_landmarks
    mp, frames, rows = plan.morph, plan.frames, plan.rows
    S, K, dev, M, m = det.S, det.K, det.dev, mp.M, mp.anchors
    F, T, B = len(rows), len(frames), mp.ring
    matched, hull, seam = bool(mp.colour.any()), mp.mask == 'hull', bool(mp.seamless.any())
    filter_gain, filter_diff = matched and plan.colour_smooth < 1.0, seam and plan.seam_smooth < 1.0
    max_pixels = grid_pixels(rows)
    held = _Held(dev)                                          # what the loop's _join records: every tensor made below
    up, empty = held.up, held.empty
    with torch.cuda.device(dev):
        # once per call, on the caller's stream: the donors, their landmarks, the links and the per-face settings
        lm_b = held.keep(pose_landmarks(det, ('photos', mp.donors, mp.donor_rows_given) if mp.donor_landmarks is None else
                                        ('landmarks', mp.donor_landmarks), F).contiguous())
        don, doffs_d, dhw_d, dboxes_d = held.keep(*pack_u8(mp.donors, dev, mp.donor_rows))
        links_d, shape_d, texture_d = up(compose_links(rows)), up(mp.shape), up(mp.texture)
        anchors_d = up(WP.warp_anchors(m).astype(np.float32)) if m else None
        own, fit_flags, inv_ramp = empty(T, F, K, 2), empty(T, F, dtype=torch.int32), empty(T, F, 2)
        poses2, mu2 = empty(2, F, K, 2), empty(2, F, K, 2)
        coef2, ctrl2, flags2 = empty(2, F, M + 3, 2), empty(2, F, M, 2), empty(2, F, dtype=torch.int32)
        gain = cflags = hflags = diff = sflags = inv_soft = feather_d = None
        if matched:
            colour_d, sums_a, sums_b = up(mp.colour), empty(F, 7, dtype=torch.int64), empty(F, 7, dtype=torch.int64)
            gain, cflags = empty(T, F, 3, 2), empty(T, F, dtype=torch.int32)
            gain_state, gain_seen = empty(F, 6), held.zeros(F, dtype=torch.int32)
        if hull:
            grow_d, feather_d = up(mp.grow), up(mp.mask_feather)
            inv_soft, edges, hflags = empty(T, F), empty(F, K, 3), empty(T, F, dtype=torch.int32)
        if seam:
            seamless_d, dirs_d = up(mp.seamless), up(MP.seam_dirs(B))
            ring, diff, sflags = empty(F, B, 2), empty(T, F, B, 3), empty(T, F, dtype=torch.int32)
            diff_state, diff_seen = empty(F, 3 * B), held.zeros(F, dtype=torch.int32)
        if matched:                                            # once per call, behind a fork of its own: the donors' sums
            det._fork()
            with torch.cuda.stream(det.stream):
                ops.colour_stats_u8(don, doffs_d, dhw_d, dboxes_d, int(box_areas(mp.donor_rows).max()), sums_b)

    def frame(t, f):
        b, fsrc, foffs_d, fhw_d = f.bufs, f.src, f.offs, f.hw
        rows_t, lost_t = b['boxes'][t], b['flags'][t]
        ops.clip_rows(rows_t, lost_t, b['mu'][t], b['smooth'][t] if plan.smooth else None, S, mp.feather, feather_d, own[t], inv_ramp[t],
                      inv_soft[t] if hull else None)
        extra = {}
        if matched:
            ops.colour_stats_u8(fsrc, foffs_d, fhw_d, rows_t, max_pixels, sums_a)
            ops.colour_gain(sums_a, sums_b, colour_d, mp.max_gain, gain[t], cflags[t])
            if filter_gain:
                ops.clip_ema(gain[t].view(F, 6), gain_state, gain_seen, cflags[t], lost_t, plan.colour_smooth)
            extra['gain'] = gain[t]
        ops.morph_poses(own[t], lm_b, shape_d, poses2, mu2)
        if hull:                                               # the blended landmarks, read in place
            ops.hull_fit(poses2[0], rows_t, grow_d, edges, hflags[t])
            extra['edges'], extra['inv_soft'] = edges, inv_soft[t]
        ops.warp_fit(poses2.view(2 * F, K, 2), mu2.view(2 * F, K, 2), anchors_d, 1.0, mp.lam, coef2.view(2 * F, M + 3, 2),
                     ctrl2.view(2 * F, M, 2), flags2.view(2 * F))
        torch.bitwise_or(flags2[0], flags2[1], out=fit_flags[t])
        if seam:
            ops.seam_fit(poses2[0], rows_t, grow_d, edges, hflags[t], dirs_d, fsrc, foffs_d, fhw_d, don, doffs_d, dhw_d, dboxes_d,
                         texture_d, ctrl2[0], coef2[0], coef2[1], gain[t] if matched else None, ring, diff[t], sflags[t])
            if filter_diff:
                ops.clip_ema(diff[t].view(F, 3 * B), diff_state, diff_seen, sflags[t], lost_t, plan.seam_smooth)
            extra['ring'], extra['diff'], extra['seamless'] = ring, diff[t], seamless_d
        ops.morph_paste(fsrc, f.canvas, foffs_d, fhw_d, don, doffs_d, dhw_d, rows_t, dboxes_d, links_d, inv_ramp[t], texture_d,
                        ctrl2[0], coef2[0], coef2[1], max_pixels, **extra)

    tracker = TR.FaceTracker(det, None, plan.box_smooth, plan.one_euro, plan.fps, capacity=T, gate=plan.gate)
    out = TR.run_frames(det, frames, plan.chunk_frames, held, frame, tracker, rows)
    return ClipMorph(out, tracker.result(), own, fit_flags, gain, cflags, hflags, diff, sflags)
