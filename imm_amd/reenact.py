"""Re-enactment: a tracked driving clip animates the faces of still photos.

    r = gen.reenact(photos, frames, driver_box, boxes)     # photos: u8 arrays, boxes: their n faces; frames: T u8 arrays,
    r.frames[t][i]                                         # driver_box: the ONE driving face of frames[0]; photo i at frame t, u8
    r.landmarks, r.flags, r.held, r.faces, r.track         # f32 [T, n, K, 2], int32 [T, n], bool [T, n], f32 [T, n, S, S, 3], a Track

Once per call the photos are packed and uploaded, the n boxes cut (imm_resize_crop_u8), the appearance stage of the generator run (its
features stay in the joint buffer: the render stage writes the Gaussian-map channels only) and the faces' own landmarks m detected.
Per frame, without anything returning to the host between the clip's first and last launch:

    detector's stream     the tracker's frame (FaceTracker._advance with the one driver face: crop, pose program, imm_track_step, copy)
                          imm_retarget: that frame's points_smooth (or points) and flags -> landmarks[t]; a held face keeps landmarks[t - 1]
    generator's stream    waits for the detector's; landmarks[t] -> the render stage's input; the captured render program of the bucket;
                          the packed photos copied into slot t of the result and one imm_compose_u8 launch into it

include/imm_retarget.h states once how a driver's landmarks become the pose of a different face: the similarity of the driver's
first-frame shape onto the face's own landmarks carries the driver's motion since its first frame ('relative') or its shape itself
('absolute') into the face's box; rigid=False first divides the driver's head motion out, so that only its expression moves the face.

This module holds the host side: plan_reenact (every argument checked before anything reaches the device), Reenactment (the result)
and run (the launches).  It imports without a GPU."""
import math

import numpy as np
import torch

from . import tracking as TR
from .inference import _Plan

MOTIONS = ('relative', 'absolute')
FLAG_HELD = 1
GAIN_MAX = 4.0


def check_motion(motion):
    if motion not in MOTIONS:
        raise ValueError('motion must be one of %s, got %r' % (', '.join(repr(m) for m in MOTIONS), motion))
    return motion


def check_gain(gain):
    g = float(gain)
    if not (math.isfinite(g) and 0.0 <= g <= GAIN_MAX):
        raise ValueError('gain must be finite and lie in [0, %g], got %r' % (GAIN_MAX, gain))
    return g


def check_driver_box(driver_box):
    """The ONE driving face of the clip's first frame as an int32 row [1, 5]: (y0, x0, y1, x1), (0, y0, x0, y1, x1) or a list of one such."""
    box = driver_box
    if isinstance(box, np.ndarray):
        box = box.tolist()
    if isinstance(box, (list, tuple)) and len(box) in (4, 5) and all(np.isscalar(v) for v in box):
        box = [box]
    if not isinstance(box, (list, tuple)):
        raise ValueError('driver_box must be the box (y0, x0, y1, x1) of the one driving face of frames[0], got %r' % (driver_box,))
    if len(box) != 1:
        raise ValueError('%d driver faces: re-enactment follows ONE driving face (several drivers are not implemented); give the box '
                         '(y0, x0, y1, x1) of that face in frames[0]' % len(box))
    return TR.check_first_boxes(box, 'frames[0]')


class ReenactPlan(_Plan):
    """reenact()'s checked arguments."""
    FIELDS = ('photos', 'rows', 'frames', 'driver_row', 'relative', 'rigid', 'gain', 'smooth', 'feather', 'paste', 'box_smooth', 'one_euro',
              'fps', 'chunk_frames')


def plan_reenact(photos, frames, driver_box, boxes=None, max_batch=128, motion='relative', rigid=True, gain=1.0, smooth=True,
                 feather=0.125, paste=True, box_smooth=0.5, one_euro=TR.OneEuro(), fps=25.0, chunk_frames=32, template=None, model=None):
    """reenact()'s arguments checked on the host, before anything reaches the device: a ReenactPlan of the photos as decoded u8 arrays,
    their box rows int32 [n, 5], the frames as decoded u8 arrays, the driver's row int32 [1, 5], and the checked settings."""
    from .generation import NEEDS_U8, check_feather
    from .inference import photos_and_rows
    if template is not None:
        raise NotImplementedError('reenact with a template (re-enactment in the aligned frame) is not implemented: the faces are '
                                  'rendered in their raw box crops')
    if model is not None:
        raise NotImplementedError('reenact carries the driver\'s motion over with a similarity; model=%r (the tps and affine models) '
                                  'is not implemented' % (model,))
    motion, gain, feather = check_motion(motion), check_gain(gain), check_feather(feather)
    photos, rows = photos_and_rows(photos, boxes, NEEDS_U8, 'no photos', not_u8=ValueError)
    if len(rows) > int(max_batch):
        raise ValueError('%d faces, the generator\'s max_batch is %d' % (len(rows), int(max_batch)))
    drow = check_driver_box(driver_box)
    frames, drow, beta, consts, chunk = TR.plan_track(frames, drow, max_batch, box_smooth, one_euro, fps, chunk_frames)
    return ReenactPlan(photos=photos, rows=rows, frames=frames, driver_row=drow, relative=motion == 'relative', rigid=bool(rigid), gain=gain,
                       smooth=bool(smooth), feather=feather, paste=bool(paste), box_smooth=beta, one_euro=one_euro, fps=float(fps),
                       chunk_frames=chunk)


class Reenactment(object):
    """What reenact returns, T frames by n source faces, tensors on the generator's device:
    landmarks f32 [T, n, K, 2] the poses rendered ((y, x) in [-1, 1] of each face's box); flags int32 [T, n] (bit 0 held: the pose of
    the frame before was kept); faces f32 [T, n, S, S, 3] the generated faces, or None; frames: with paste, frames[t][i] is photo i at
    frame t, u8 [h_i, w_i, 3], views of one [T, packed] device buffer, else None; track: the driver's tracking.Track."""

    def __init__(self, landmarks, flags, faces, frames, track):
        self.landmarks, self.flags, self.faces, self.frames, self.track = landmarks, flags, faces, frames, track

    def __len__(self):
        return int(self.landmarks.shape[0])

    @property
    def held(self):
        """bool [T, n]: the driver was lost on that frame or the rule had no usable answer for that face; its pose was kept."""
        return (self.flags & FLAG_HELD) != 0


def check_render_keeps_features(gen, bucket):
    """The appearance features of a bucket survive its render stage: the stage's first launch writes the Gaussian maps into the joint
    buffer's channels [8f, 8f + K) and every later one writes an activation or the prediction buffer."""
    prog = gen.program('render', bucket)
    if prog[0].tag != 'gauss' or any(l.tag not in ('conv', 'upsample') for l in prog[1:]):
        raise RuntimeError('the render stage of this generator writes more of the joint buffer than the Gaussian maps: %s' % (
            [l.tag for l in prog],))


def run(gen, plan, return_faces=False):
    """The launches of reenact() for a checked plan (see the module docstring); called with the caller's stream current.  The frame
    loop is tracking.run_frames, without a canvas; `frame` is the retargeting behind the tracker's launches and the generator's half."""
    from . import ops
    from .generation import PasteSetup
    from .inference import _Held, pack_u8, plan_buckets, unpack_u8
    det, S, K, dev = gen.detector, gen.S, gen.K, gen.dev
    photos, rows, frames = plan.photos, plan.rows, plan.frames
    n, T = len(rows), len(frames)
    buckets = plan_buckets(n, gen.max_batch)                   # one: n <= max_batch
    bucket = buckets[0][2]
    held = _Held(dev)                                          # what both _joins record: every tensor made below
    with torch.cuda.device(dev):
        if plan.paste:
            ps = PasteSetup(photos, rows, buckets, plan.feather, dev, clone=False)      # all photos, once per call
            held.keep(*ps.tensors())
            packed, max_pixels = ps.packed(slice(None)), ps.max_pixels(slice(None))
            canvas = held.empty(T, ps.src.numel(), dtype=torch.uint8)
        else:
            packed = held.keep(*pack_u8(photos, dev, rows))
        src, offs_d, hw_d, boxes_d = packed
        m, lm, flags = held.empty(n, K, 2), held.empty(T, n, K, 2), held.empty(T, n, dtype=torch.int32)
        anchor = held.zeros(K, 2, dtype=torch.float64)
        faces = held.empty(T, n, S, S, 3) if return_faces else None
        # once per call, on the detector's stream: the faces' own landmarks (detector.landmarks(photos, boxes), from the packed photos)
        cur = det._fork()
        with torch.cuda.stream(det.stream):
            det._stage(n, bucket, packed=packed)
            det._run(bucket)
            m.copy_(det._mu[:n])
        # once per call, on the generator's stream: the appearance of every face, which stays in the joint buffer
        gen._fork()
        with torch.cuda.stream(gen.stream):
            gen._ensure_capacity(bucket)
            check_render_keeps_features(gen, bucket)
            gen._stage(n, bucket, packed=packed)
            gen._mu[:bucket].zero_()
            gen._capture('render', bucket)                     # capture (and its synchronisation) ahead of the first frame
            gen._run('appearance', bucket)
    which = 'smooth' if plan.smooth else 'points'

    def frame(t, f):
        b = f.bufs
        ops.retarget(b[which][t, 0], anchor, b['flags'][t], m, lm[t - 1] if t else m, int(t == 0), plan.relative, plan.rigid,
                     plan.gain, lm[t], flags[t])
        gen.stream.wait_stream(det.stream)
        with torch.cuda.stream(gen.stream):
            gen._mu[:n].copy_(lm[t])
            gen._run('render', bucket)
            if plan.paste:
                canvas[t].copy_(src)
                ops.compose_u8(canvas[t], offs_d, hw_d, boxes_d, ps.links_d, ps.ramp_d, gen._pred[:n], max_pixels)
            if return_faces:
                faces[t].copy_(gen._pred[:n, ..., :3])

    tracker = TR.FaceTracker(det, None, plan.box_smooth, plan.one_euro, plan.fps, capacity=T)
    TR.run_frames(det, frames, plan.chunk_frames, held, frame, tracker, plan.driver_row, canvas=False)
    gen._join(cur, *held)
    out = None
    if plan.paste:
        out = [unpack_u8(canvas[t], photos) for t in range(T)]
    return Reenactment(lm, flags, faces, out, tracker.result())
