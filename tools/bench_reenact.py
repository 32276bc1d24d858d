"""Frames/s of re-enactment: ImageGenerator.reenact (photos uploaded, cut and encoded once; per frame the tracker, imm_retarget, the
render program and one imm_compose_u8 launch, nothing returning to the host) against the loop a user writes without it:
detector.track(clip, [driver_box]), .cpu(), the rule of include/imm_retarget.h in vectorised numpy on the host, and
repose(photos, landmarks_t, boxes) per frame.  64 driver frames of 512 x 384, n = 1, 4, 16 source faces of 160 x 128 px in
photos of 512 x 384, S = 128, K = 10, bf16; writes the table to profiles/reenact_bench.txt.

Both sides are wall-clock times of the whole clip, from the call to a final synchronisation.  After untimed warm-up runs of both, the
two sides alternate, one clip each per window; the table gives the median and the range over the windows.  Before the timed windows
the two sides' landmarks are compared (the host rule is numpy's own summation order, not the bit-exact restatement of the tests).
Usage: python tools/bench_reenact.py [--faces 1 4 16] [--frames 64] [--windows 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imm_amd.models.imm_model import IMMModel             # noqa: E402
from imm_amd.tracking import OneEuro                      # noqa: E402
from bench_detect import model_config                     # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'reenact_bench.txt')
DRIVER = (40, 60, 360, 316)
# launches issued per frame by reenact(): the tracker's four (imm_resize_crop_u8, the captured pose program, imm_track_step, the copy
# of the landmarks), imm_retarget, the copy into the render stage's input, the captured render program, the copy of the packed
# photos into the frame's slot and imm_compose_u8
LAUNCHES_PER_FRAME = 9


def host_retarget(q, q0, m, relative=True, rigid=True, gain=1.0):
    """The rule of include/imm_retarget.h for one frame in vectorised numpy f64 (complex arithmetic, numpy's own summation order):
    q, q0 [K, 2], m [n, K, 2] -> [n, K, 2] f32, or None where a face would be held."""
    z, zq, zm = q0[:, 0] + 1j * q0[:, 1], q[:, 0] + 1j * q[:, 1], m[..., 0].astype(np.float64) + 1j * m[..., 1]
    u = z - z.mean()
    den = (np.abs(u) ** 2).sum()
    a = (np.conj(u) * (zm - zm.mean(1, keepdims=True))).sum(1) / den
    zt = zq
    if not rigid:
        b = (np.conj(u) * (zq - zq.mean())).sum() / den
        zt = z.mean() + (zq - zq.mean()) / b
    t = zm + a[:, None] * (zt - z) if relative else zm.mean(1, keepdims=True) + a[:, None] * (zt - z.mean())
    o = zm + gain * (t - zm)
    out = np.clip(np.stack([o.real, o.imag], -1), -1.0, 1.0).astype(np.float32)
    held = ~np.isfinite(out).all((1, 2)) | (a == 0)
    out[held] = np.nan
    return out, held


def user_loop(gen, photos, boxes, frames, oe, fps):
    tr = gen.detector.track(frames, [DRIVER], box_smooth=0.5, one_euro=oe, fps=fps).cpu()
    m = gen.detector.landmarks(photos, boxes).cpu().numpy()
    pts, lost = tr.points_smooth[:, 0].numpy().astype(np.float64), tr.lost[:, 0].numpy()
    prev, out, lms = m, [], []
    for t in range(len(frames)):
        lm, held = host_retarget(pts[t], pts[0], m)
        held |= bool(lost[t])
        lm[held] = prev[held]
        out.append(gen.repose(photos, torch.from_numpy(lm), boxes))
        lms.append(lm)
        prev = lm
    return out, np.stack(lms)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    del r
    return (time.perf_counter() - t0) * 1e3


def main(args):
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    S, K, T = 128, 10, args.frames
    rng = np.random.RandomState(0)
    base = rng.randint(0, 256, size=(512 + T, 384 + T, 3)).astype(np.uint8)
    frames = [np.ascontiguousarray(base[t:t + 512, T - t:T - t + 384]) for t in range(T)]      # the clip slides a pixel per frame
    props = torch.cuda.get_device_properties(0)
    lines = ['device: %s (%s, %d CUs)' % (props.name, props.gcnArchName, props.multi_processor_count),
             'S %d, K %d, bf16; %d u8 driver frames of 512 x 384, one driving face; n source faces of 160 x 128 px in photos of 512 x 384 '
             '(four faces a photo); motion relative, rigid, gain 1, feather 0.125, box_smooth 0.5, OneEuro(), 25 fps' % (S, K, T),
             'wall-clock ms per clip, the two sides alternating, median (min .. max) of %d windows after %d warm-up clips each' % (
                 args.windows, args.warmup),
             'loop    = track(clip, [box]), .cpu(), the rule in numpy on the host, repose(photos, landmarks_t, boxes) per frame',
             'reenact = ImageGenerator.reenact(photos, clip, box, boxes, chunk_frames=32): %d launches per frame, no copy to the host' %
             LAUNCHES_PER_FRAME,
             '%4s %32s %32s %12s %14s %8s' % ('n', 'loop ms', 'reenact ms', 'loop fr/s', 'reenact fr/s', 'ratio')]
    rows = []
    for n in args.faces:
        n_photos = (n + 3) // 4
        photos = [rng.randint(0, 256, size=(512, 384, 3)).astype(np.uint8) for _ in range(n_photos)]
        boxes = [(i // 4, 20 + 90 * (i % 4), 10 + 60 * (i % 4), 180 + 90 * (i % 4), 138 + 60 * (i % 4)) for i in range(n)]
        model = IMMModel(model_config(K), dtype=torch.bfloat16, device=dev)
        x = torch.zeros(max(n, 2), S, S, 3, device=dev)
        model.build({'image': x, 'future_image': x}, training_pl=False, build_loss=False)
        gen = model.image_generator(S, max_batch=max(n, 1))
        oe = OneEuro()
        loop = lambda: user_loop(gen, photos, boxes, frames, oe, 25.0)
        fused = lambda: gen.reenact(photos, frames, DRIVER, boxes, one_euro=oe, fps=25.0, chunk_frames=32)
        for _ in range(args.warmup):
            loop()
            fused()
        out_l, lm_l = loop()
        r = fused()
        torch.cuda.synchronize()
        lm_err = float(np.abs(r.landmarks.cpu().numpy() - lm_l).max())
        px_diff = max(int((a.cpu().numpy().astype(np.int32) - b.cpu().numpy()).__abs__().max()) for fa, fb in zip(out_l, r.frames)
                      for a, b in zip(fa, fb))
        del out_l, r
        t_loop, t_fused = [], []
        for _ in range(args.windows):
            t_loop.append(wall_ms(loop))
            t_fused.append(wall_ms(fused))
        ml, mf = float(np.median(t_loop)), float(np.median(t_fused))
        row = {'faces': n, 'frames': T, 'loop_ms': ml, 'reenact_ms': mf, 'loop_ms_all': t_loop, 'reenact_ms_all': t_fused,
               'loop_frames_per_s': T / ml * 1e3, 'reenact_frames_per_s': T / mf * 1e3, 'loop_over_reenact': ml / mf,
               'landmarks_max_abs_diff': lm_err, 'pixels_max_abs_diff': px_diff, 'launches_per_frame': LAUNCHES_PER_FRAME}
        rows.append(row)
        fmt = lambda v: '%8.2f (%8.2f .. %8.2f)' % (float(np.median(v)), min(v), max(v))
        lines.append('%4d %32s %32s %12.0f %14.0f %8.2f   max |landmarks diff| %.1e, max |u8 diff| %d' % (
            n, fmt(t_loop), fmt(t_fused), row['loop_frames_per_s'], row['reenact_frames_per_s'], row['loop_over_reenact'], lm_err, px_diff))
        print(lines[-1], flush=True)
        del gen, model
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)
    print(json.dumps({'image_size': S, 'n_maps': K, 'dtype': 'bf16', 'rows': rows}))


if __name__ == '__main__':
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--faces', type=int, nargs='+', default=[1, 4, 16])
    p.add_argument('--frames', type=int, default=64)
    p.add_argument('--windows', type=int, default=7)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--out', type=str, default=OUT)
    main(p.parse_args())
