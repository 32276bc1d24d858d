"""Face tracking: the boxes follow the landmarks from frame to frame.

Every program of the detector works on a face box per row.  For a clip the caller has the boxes of its first frame only; here the
box of every later frame comes from the landmarks of the frame before it, on the device:

    tr = det.track(frames, boxes)                       # frames: T u8 HWC arrays, boxes: the faces of frames[0]
    tr.points, tr.points_smooth                         # f32 [T, F, K, 2] source pixels (y, x); tr.boxes int32 [T, F, 4]; tr.lost
    tr = det.tracker(gate=gate).track(frames, boxes)    # a quality.QualityGate: a face that fails it on a frame is lost there (tr.unsure)
    live = det.tracker(); live.start(frame0, boxes); live.step(frame1); ...; live.result()

Per frame, on the detector's stream: imm_resize_crop_u8 with the box rows in device memory, the captured pose program of the bucket,
imm_track_step (include/imm_track.h states the rule once: landmarks -> source pixels -> similarity fit of the first frame's shape ->
box filter -> the next frame's box row and geometry -> One-Euro filter of the points), and a device copy of the landmarks into the
result.  Nothing comes back to the host between a clip's first and last launch.

With a gate (imm_amd/quality.py) one launch stands between the pose program and imm_track_step: imm_landmark_scores (include/imm_score.h)
scores the frame's faces from the soft-argmax marginals and from the first frame's shape in the tracker's state, and hands imm_track_step
NaN landmarks for a face that fails the gate's thresholds.  The lost rule of imm_track.h does the rest: the face keeps its state, box and
filter pairs, its points are NaN and FLAG_LOST is set.  Without a gate the launches, arguments and buffers are those of before.

This module holds the host side: OneEuro (the filter's constants), plan_track (every argument checked before anything reaches the
device), the state layout, Track (the result), FaceTracker (the launches of a frame) and run_frames, the one frame loop under track and
under every clip operation built on the tracker (morph_clip, redact_clip, annotate_clip, reenact).  It imports without a GPU."""
import math

import numpy as np
import torch

from . import keypoints as KP

STATE_HEAD = 5                # h0, w0, cy, cx, s in front of z0, xhat, dxhat (include/imm_track.h)
FLAG_LOST, FLAG_OUTSIDE = 1, 2
FLAG_UNSURE = 4               # not the tracker's: the bit under which a clip operation ORs the gate's verdict into its flags (or_unsure)


def or_unsure(flags, qflags):
    """flags |= FLAG_UNSURE where the gate's verdict qflags is not 0, in place on the device (int32, one value per face)."""
    return flags.bitwise_or_(qflags.ne(0).to(torch.int32).mul_(FLAG_UNSURE))


def state_size(K):
    """f64 values of one face's state: (h0, w0, cy, cx, s), then z0, xhat, dxhat [K, 2] each."""
    return STATE_HEAD + 6 * int(K)


def state_views(state, K):
    """One face's (or [F, ..] faces') state split into named views: h0w0 [.., 2], box [.., 3] = (cy, cx, s), z0, xhat, dxhat [.., K, 2]."""
    K = int(K)
    lead = state.shape[:-1]
    part = lambda i: state[..., STATE_HEAD + 2 * K * i:STATE_HEAD + 2 * K * (i + 1)].reshape(lead + (K, 2))
    return {'h0w0': state[..., 0:2], 'box': state[..., 2:5], 'z0': part(0), 'xhat': part(1), 'dxhat': part(2)}


class OneEuro(object):
    """The constants of the One-Euro filter (Casiez, Roussel, Vogel 2012) of the tracked points: the cutoff of the low-pass is
    min_cutoff + beta * |speed| Hz, the speed (in box heights per second) itself low-passed at d_cutoff Hz.  Conventional values;
    they are not tuned against video here."""

    def __init__(self, min_cutoff=1.0, beta=0.05, d_cutoff=1.0):
        self.min_cutoff, self.beta, self.d_cutoff = float(min_cutoff), float(beta), float(d_cutoff)
        for name in ('min_cutoff', 'd_cutoff'):
            v = getattr(self, name)
            if not (math.isfinite(v) and v > 0):
                raise ValueError('%s must be finite and positive, got %r' % (name, v))
        if not (math.isfinite(self.beta) and self.beta >= 0):
            raise ValueError('beta must be finite and >= 0, got %r' % (self.beta,))

    def __repr__(self):
        return 'OneEuro(min_cutoff=%g, beta=%g, d_cutoff=%g)' % (self.min_cutoff, self.beta, self.d_cutoff)


def filter_constants(one_euro, fps):
    """(min_cutoff, beta, d_cutoff, c, te, filter_off) as imm_track_step takes them: c = 2 pi / fps and te = 1 / fps formed here in f64,
    so no transcendental constant is formed on the device.  one_euro None: the filter is off (neutral constants are passed)."""
    fps = float(fps)
    if not (math.isfinite(fps) and fps > 0):
        raise ValueError('fps must be finite and positive, got %r' % (fps,))
    off = one_euro is None
    oe = OneEuro() if off else one_euro
    if not isinstance(oe, OneEuro):
        raise ValueError('one_euro must be a tracking.OneEuro or None, got %r' % (one_euro,))
    return oe.min_cutoff, oe.beta, oe.d_cutoff, 2.0 * math.pi / fps, 1.0 / fps, int(off)


def check_box_smooth(box_smooth):
    b = float(box_smooth)
    if not (0.0 < b <= 1.0):
        raise ValueError('box_smooth must lie in (0, 1], got %r' % (box_smooth,))
    return b


def check_first_boxes(boxes, what='frame 0'):
    """The faces of a clip's first frame as int32 rows [F, 5] (0, y0, x0, y1, x1): keypoints.check_boxes against that one frame.
    Rows of four values are all faces of that frame.  ValueError for a row naming another frame."""
    rows = [list(b) for b in boxes]
    if rows and all(len(r) == 4 for r in rows):
        rows = [[0] + r for r in rows]
    try:
        return KP.check_boxes(rows, 1)
    except ValueError as e:
        if 'names image' in str(e):
            raise ValueError('%s: every box row must name %s (image index 0)' % (e, what))
        raise


def plan_track(frames, boxes, n_faces_max, box_smooth=0.5, one_euro=OneEuro(), fps=25.0, chunk_frames=32, gate=None):
    """track()'s arguments checked on the host, before anything reaches the device: (frames as decoded u8 arrays, box rows int32
    [F, 5], box_smooth, filter constants (filter_constants), chunk_frames).  n_faces_max: the detector's max_batch.  gate: None or a
    quality.QualityGate (ValueError otherwise)."""
    from .inference import decode_u8
    from .quality import check_gate
    check_gate(gate)
    if not isinstance(frames, (list, tuple)):
        raise ValueError('track needs the frames as a list of u8 HWC arrays (a tensor batch holds no photo to cut boxes from)')
    if len(frames) == 0:
        raise ValueError('no frames')
    try:
        frames = decode_u8(frames)
    except TypeError as e:
        raise ValueError(str(e))
    rows = check_first_boxes(boxes)
    if len(rows) > int(n_faces_max):
        raise ValueError('%d faces, the detector\'s max_batch is %d' % (len(rows), int(n_faces_max)))
    chunk = int(chunk_frames)
    if chunk < 1:
        raise ValueError('chunk_frames must be >= 1, got %r' % (chunk_frames,))
    return frames, rows, check_box_smooth(box_smooth), filter_constants(one_euro, fps), chunk


class Track(object):
    """What tracking returns, T frames by F faces, tensors on the detector's device (or the host after .cpu()):
    mu f32 [T, F, K, 2] the landmarks (y, x) in [-1, 1] of each frame's box; points f32 [T, F, K, 2] the same in source pixels;
    points_smooth f32 [T, F, K, 2] after the One-Euro filter; boxes int32 [T, F, 4] the box (y0, x0, y1, x1) each frame was cut
    with; flags int32 [T, F] (bit 0 lost, bit 1 the next box left the photo); keypoints f32 [T, F, M, 2] with a regressor, else None.
    Tracked with a gate (quality.QualityGate), also spread f32 [T, F, K], score f32 [T, F, 2] = (mean spread, shape residual against the
    first frame's shape; 0 on frame 0) and qflags int32 [T, F] (bit 0: the spread failed the gate, bit 1: the residual did); else None."""

    def __init__(self, mu, points, points_smooth, boxes, flags, keypoints=None, spread=None, score=None, qflags=None):
        self.mu, self.points, self.points_smooth, self.boxes, self.flags, self.keypoints = mu, points, points_smooth, boxes, flags, keypoints
        self.spread, self.score, self.qflags = spread, score, qflags

    def __len__(self):
        return int(self.mu.shape[0])

    @property
    def lost(self):
        """bool [T, F]: the fit of that frame was unusable (a non-finite landmark, a degenerate shape); the box was kept."""
        return (self.flags & FLAG_LOST) != 0

    @property
    def outside(self):
        """bool [T, F]: the box made from that frame does not intersect the photo the frame was cut from."""
        return (self.flags & FLAG_OUTSIDE) != 0

    @property
    def unsure(self):
        """bool [T, F]: a quality score of that frame failed the gate (all False when tracked without a gate).  On every frame but the
        first such a face is also lost; on the first frame it is scored but kept: the caller vouches for the first boxes."""
        return (self.flags & 0) != 0 if self.qflags is None else self.qflags != 0

    def cpu(self):
        from . import ops
        get = lambda t: None if t is None else ops.download(t.contiguous())
        return Track(get(self.mu), get(self.points), get(self.points_smooth), get(self.boxes), get(self.flags), get(self.keypoints),
                     spread=get(self.spread), score=get(self.score), qflags=get(self.qflags))


class FaceTracker(object):
    """Tracking of live input: start(frame, boxes) with the faces of the first frame, then step(frame) per frame; result() is the
    Track of the frames seen so far (views of the tracker's buffers).  LandmarkDetector.track is start + step over a clip with the
    frames uploaded chunk_frames at a time.
    Every frame is issued on the detector's stream without a device -> host copy and without synchronising that stream; the host
    waits only for its own uploads, on a side stream.  With a regressor the geometry rows of the detector (the keypoint epilogue's
    input) are written by each frame for the next one: keypoints() or align() calls on the same detector between two steps of such a
    tracker overwrite them.
    gate: a quality.QualityGate (its thresholds possibly both None: the frames are then scored and nothing is blanked), or None: no
    scores, and exactly the launches of a tracker without this argument."""

    def __init__(self, detector, regressor=None, box_smooth=0.5, one_euro=OneEuro(), fps=25.0, capacity=64, gate=None):
        from .quality import check_gate
        self.gate = check_gate(gate, detector.K, detector.S)
        self.det = detector
        self.reg = regressor
        if regressor is not None:
            regressor.check(detector.K, detector.S)
            regressor.epilogue_weights()
        self.box_smooth = check_box_smooth(box_smooth)
        self.consts = filter_constants(one_euro, fps)
        self.capacity = max(1, int(capacity))
        self.t = 0
        self.F = 0

    # ------------------------------------------------------------------------------------------------------------------------
    def _alloc(self, cap):
        det, F, K = self.det, self.F, self.det.K
        dev = det.dev
        bufs = {'mu': torch.empty(cap, F, K, 2, device=dev), 'points': torch.empty(cap, F, K, 2, device=dev),
                'smooth': torch.empty(cap, F, K, 2, device=dev), 'flags': torch.empty(cap, F, dtype=torch.int32, device=dev),
                'boxes': torch.zeros(cap + 1, F, 5, dtype=torch.int32, device=dev)}
        if self.reg is not None:
            bufs['kp'] = torch.empty(cap, F, self.reg.M, 2, device=dev)
        if self.gate is not None:
            bufs.update(spread=torch.empty(cap, F, K, device=dev), score=torch.empty(cap, F, 2, device=dev),
                        qflags=torch.empty(cap, F, dtype=torch.int32, device=dev))
        return bufs

    def _grow(self):
        """Twice the frames (device copies on the detector's stream, which is current; the old buffers stay valid for results handed
        out).  The new buffers are read on the caller's stream later: the allocator is told."""
        old, t = self._bufs, self.t
        self.capacity *= 2
        new = self._alloc(self.capacity)
        for k, v in old.items():
            n = t + 1 if k == 'boxes' else t
            new[k][:n].copy_(v[:n])
            new[k].record_stream(self._cur)
        self._bufs = new

    def _upload(self, frames):
        """Decoded u8 frames packed into one device buffer on the upload stream: (src, offsets, hw, count).  The detector's stream
        waits for the copies on the device."""
        from .inference import pack_u8
        det = self.det
        up = getattr(det, '_upload_stream', None)
        if up is None:
            up = det._upload_stream = torch.cuda.Stream(device=det.dev)
        with torch.cuda.device(det.dev), torch.cuda.stream(up):
            src, offs_d, hw_d, _ = pack_u8(frames, det.dev)
        det.stream.wait_stream(up)
        for t in (src, offs_d, hw_d):
            t.record_stream(det.stream)
        return src, offs_d, hw_d, len(frames)

    def _begin(self, rows):
        """Buffers, the first frame's box rows and geometry, the regressor's weights and the bucket's captured program: everything
        that is not a per-frame launch.  Called with the caller's stream current."""
        from .inference import plan_buckets
        det = self.det
        self.F = F = len(rows)
        if F > det.max_batch:
            raise ValueError('%d faces, the detector\'s max_batch is %d' % (F, det.max_batch))
        self.bucket = plan_buckets(F, det.max_batch)[0][2]
        self.M = None if self.reg is None else self.reg.M
        self.t = 0
        with torch.cuda.device(det.dev):
            self._bufs = self._alloc(self.capacity)
            self._state = torch.zeros(F, state_size(det.K), dtype=torch.float64, device=det.dev)
            if self.gate is not None:                      # what imm_track_step reads in place of the detector's landmarks
                self._mu_gated = torch.empty(F, det.K, 2, device=det.dev)
            det._fork()
            with torch.cuda.stream(det.stream):
                det._ensure_capacity(self.bucket)
                det._stager.copy(self._bufs['boxes'][0], torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)), ('track_rows', F))
                if self.reg is not None:
                    w, b = self.reg.epilogue_weights()
                    det._stager.copy(det._kp_w[:w.size], torch.from_numpy(w.reshape(-1)), ('kp_w', self.M))
                    det._stager.copy(det._kp_b[:b.size], torch.from_numpy(b), ('kp_b', self.M))
                    det._stager.copy(det._geom[:F], torch.from_numpy(KP.box_geometry(rows, det.S)), ('geom', F))
                det._capture(self.bucket, self.M)              # capture (and its synchronisation) ahead of the first frame

    def _advance(self, src, offs_d, hw_d, next_image):
        """The launches of one frame whose photo the current box rows index in (src, offs_d, hw_d); the detector's stream is current."""
        from . import ops
        det, t, F, bucket, M = self.det, self.t, self.F, self.bucket, self.M
        if t == self.capacity:
            self._grow()
        b = self._bufs
        rows = b['boxes'][t]
        det._stage(F, bucket, packed=(src, offs_d, hw_d, rows))
        det._run(bucket, M)
        mc, be, dc, c, te, off = self.consts
        mu = det._mu[:F]
        if self.gate is not None:
            # the first frame is scored only: z0 is not written yet, and the caller vouches for the first boxes
            first = t == 0
            ops.landmark_scores(det._py[:F], det._px[:F], mu, rows, None if first else self._state.view(-1)[STATE_HEAD:],
                                state_size(det.K), det.S, self.gate.max_spread, self.gate.max_residual, 0 if first else 1,
                                b['spread'][t], b['score'][t], b['qflags'][t], self._mu_gated)
            mu = self._mu_gated
        ops.track_step(mu, rows, hw_d, self._state, det.S, next_image, 1 if t == 0 else 0, self.box_smooth, mc, be, dc, c, te, off,
                       b['points'][t], b['smooth'][t], b['boxes'][t + 1], det._geom[:F], b['flags'][t])
        b['mu'][t].copy_(det._mu[:F])
        if M is not None:
            b['kp'][t].copy_(det._kp[:F * M * 2].view(F, M, 2))
        self.t = t + 1

    # ------------------------------------------------------------------------------------------------------------------------
    def start(self, frame, boxes):
        """The first frame of a clip and its faces (keypoints.check_boxes rows naming this frame, or (y0, x0, y1, x1) per face)."""
        frames, rows, _b, _c, _n = plan_track([frame], boxes, self.det.max_batch)
        self._begin(rows)
        return self._step(frames[0])

    def step(self, frame):
        """The next frame, cut with the boxes the frame before it left on the device."""
        from .inference import decode_u8
        if self.F == 0:
            raise RuntimeError('start(frame, boxes) comes first')
        try:
            frame = decode_u8([frame])[0]
        except TypeError as e:
            raise ValueError(str(e))
        return self._step(frame)

    def _step(self, frame):
        with self.det._forked() as self._cur:
            src, offs_d, hw_d, _n = self._upload([frame])
            self._advance(src, offs_d, hw_d, 0)
        return self

    def track(self, frames, boxes, chunk_frames=32):
        """A whole clip at once with this tracker's settings (its gate among them): what LandmarkDetector.track does, which takes no
        gate.  frames, boxes, chunk_frames: as LandmarkDetector.track takes them.  Returns the Track; the tracker starts afresh."""
        frames, rows, _b, _c, chunk = plan_track(frames, boxes, self.det.max_batch, chunk_frames=chunk_frames)
        self.capacity = max(self.capacity, len(frames))
        return self.run(frames, rows, chunk)

    def run(self, frames, rows, chunk_frames):
        """track(): every frame of a checked clip, uploaded chunk_frames at a time (run_frames, with no body and no canvas); the caller's
        stream waits once, at the end."""
        run_frames(self.det, frames, chunk_frames, (), None, self, rows, canvas=False)
        return self.result()

    def result(self):
        """The Track of the frames seen so far."""
        if self.F == 0:
            raise RuntimeError('start(frame, boxes) comes first')
        b, t = self._bufs, self.t
        extra = {} if self.gate is None else dict(spread=b['spread'][:t], score=b['score'][:t], qflags=b['qflags'][:t])
        return Track(b['mu'][:t], b['points'][:t], b['smooth'][:t], b['boxes'][:t, :, 1:], b['flags'][:t],
                     b['kp'][:t] if self.reg is not None else None, **extra)


class Frame(object):
    """What run_frames hands a body: the chunk's packed frames (src, offs, hw: pack_u8's), the chunk's canvas (None without one), the
    frame's index i within its chunk and bufs, the tracker's buffers as this frame's _advance left them (None without a tracker)."""
    __slots__ = ('src', 'offs', 'hw', 'canvas', 'i', 'bufs')


def run_frames(det, frames, chunk_frames, held, body, tracker=None, rows=None, canvas=True):
    """THE frame loop of track and of every clip operation (morph_clip, redact_clip, annotate_clip, reenact); called with the caller's
    stream current, behind the operation's once-per-call work.  Per chunk of chunk_frames frames one upload and, with canvas=True, one
    canvas: a device copy of the chunk, made on the detector's stream.  Per frame, with the detector's device and stream current,
    tracker._advance and then body(t, f): t the frame's index in the clip, f a Frame.  next_image of _advance is the place of the NEXT
    frame in the upload it will be read from (0 behind a chunk's last frame): the box row a frame leaves for its successor names it.
    _grow may replace the tracker's buffers in _advance, so f.bufs is taken behind it and a body takes its per-frame slot views
    (f.bufs['boxes'][t], ...) itself; nothing a later frame overwrites may be read through them.
    tracker: a fresh FaceTracker, begun here with `rows`.  ONE fork stands here, behind _begin (which forks, and may capture, on its
    own); the tracker records its grown buffers against the same stream.  An operation with once-per-call work on the detector's stream
    (clip.run's donor sums, reenact.run's own landmarks) forks a second time, in front of that work.  Without a tracker
    (annotate_clip(track=)) the chunks are packed on the caller's stream and the detector's stream waits for it once per chunk.
    held: the inference._Held of every tensor the operation made on the caller's stream; the chunks' tensors join it and the final
    _join records it.  Returns the frames of the canvases (unpack_u8: one view per frame), None with canvas=False."""
    from .inference import pack_u8, unpack_u8
    dev = det.dev
    if tracker is not None:
        tracker._begin(rows)
    cur = det._fork()
    if tracker is not None:
        tracker._cur = cur
    out, f = [] if canvas else None, Frame()
    f.canvas = f.bufs = None
    for c0 in range(0, len(frames), chunk_frames):
        chunk = frames[c0:c0 + chunk_frames]
        if tracker is not None:
            f.src, f.offs, f.hw, _ = tracker._upload(chunk)
        else:
            with torch.cuda.device(dev):
                f.src, f.offs, f.hw, _ = held.keep(*pack_u8(chunk, dev))
            det.stream.wait_stream(cur)
        if canvas:
            with torch.cuda.device(dev):
                f.canvas = held.keep(torch.empty_like(f.src))
                with torch.cuda.stream(det.stream):
                    f.canvas.copy_(f.src)
        for i in range(len(chunk)):
            with torch.cuda.device(dev), torch.cuda.stream(det.stream):
                if tracker is not None:
                    tracker._advance(f.src, f.offs, f.hw, i + 1 if i + 1 < len(chunk) else 0)
                    f.bufs = tracker._bufs
                if body is not None:
                    f.i = i
                    body(c0 + i, f)
        if canvas:
            out += unpack_u8(f.canvas, chunk)
    det._join(cur, *held)
    return out
