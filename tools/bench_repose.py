"""Faces/s of ImageGenerator.repose (u8 photos and face boxes in, the same photos out with the faces re-posed) against
ImageGenerator.render on the same rows as pre-cropped S x S tensors, at S = 128, bf16, K = 10 and one bucket of B = 64 rows: the
difference is what the crop from the photos, the packing and the compose launch cost on top of the generator.  Writes the table to
profiles/repose_bench.txt and the kernel times to profiles/repose_kernel_stats.csv.

  repose   gen.repose(photos, landmarks, boxes): pack + copy of the u8 photos, a device copy to composite into, the box crop, the
           appearance and render graphs, one imm_compose_u8 launch
  render   gen.render(crops, landmarks) on the f32 device tensor of the same boxes, cut and resized beforehand
  pack     the part of repose() that comes before any kernel: the photos packed on the host, copied to the device and copied once more
           there (inference.pack_u8 and a clone)
Both are timed with HIP events on the caller's stream, alternated window by window in the same run (median over the windows of the
mean per-call time).  The photos are about 512 x 384 (sizes vary by a few pixels) with one box of about 250 x 250 each.

The compose kernel's own time comes from a second process, `rocprofv3 --kernel-trace --stats -- python tools/bench_repose.py
--kernel-pass` (a run of its own: tracing slows the host, so no end-to-end number is taken from it).  Its algorithmic bytes are counted
from the shapes: 6 per photo pixel inside a box and the photo (3 read, 3 written) plus the three channels of every face once
(S * S * 12; at a pixel stride above 3 the cache lines fetched hold more than that); the rate is those bytes over the kernel's mean time, set against the 6.29 TB/s a float4 copy measures on this part (8 TB/s specified).
Usage: python tools/bench_repose.py [--batch 64] [--windows 7] [--reps 10]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

OUT = os.path.join(ROOT, 'profiles', 'repose_bench.txt')
STATS = os.path.join(ROOT, 'profiles', 'repose_kernel_stats.csv')
HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0
S, K = 128, 10


def scene(B, seed=0):
    """B photos of about 512 x 384 with one box of about 250 x 250 each (one in eight hangs over the photo's edge)."""
    rng = np.random.RandomState(seed)
    photos, boxes = [], []
    for i in range(B):
        h, w = 512 + int(rng.randint(-6, 7)), 384 + int(rng.randint(-6, 7))
        photos.append(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8))
        side_y, side_x = 250 + int(rng.randint(-5, 6)), 250 + int(rng.randint(-5, 6))
        y0 = int(rng.randint(0, h - side_y)) if i % 8 else h - side_y + 20
        x0 = int(rng.randint(0, w - side_x))
        boxes.append((i, y0, x0, y0 + side_y, x0 + side_x))
    lm = rng.uniform(-0.7, 0.7, size=(B, K, 2)).astype(np.float32)
    return photos, boxes, lm


def compose_bytes(photos, boxes):
    """Algorithmic bytes of one imm_compose_u8 launch over these rows: (photo bytes read + written, face bytes)."""
    px = 0
    for i, y0, x0, y1, x1 in boxes:
        h, w = photos[i].shape[:2]
        px += max(0, min(y1, h) - max(y0, 0)) * max(0, min(x1, w) - max(x0, 0))
    return 6 * px, len(boxes) * S * S * 3 * 4


def make_generator(B):
    import torch
    from bench_detect import model_config
    from imm_amd.models.imm_model import IMMModel
    torch.cuda.set_device(0)
    model = IMMModel(model_config(K), dtype=torch.bfloat16, device='cuda:0')
    x = torch.zeros(B, S, S, 3, device='cuda:0')
    model.build({'image': x, 'future_image': x}, training_pl=False, build_loss=False)          # the batch-B engine (variables)
    return model, model.image_generator(S, max_batch=B)


def kernel_pass(args):
    """What the profiled child runs: a few repose calls, nothing timed."""
    import torch
    photos, boxes, lm = scene(args.batch)
    _model, gen = make_generator(args.batch)
    lm = torch.from_numpy(lm).cuda()
    for _ in range(args.kernel_calls + 2):
        gen.repose(photos, lm, boxes)
    torch.cuda.synchronize()


def profile_kernels(args):
    """Run the kernel pass under rocprofv3 in a process of its own; returns {kernel name: [durations ns]} and writes STATS."""
    from profile_summary import rows_of, stats
    tmp = tempfile.mkdtemp(prefix='repose_prof_')
    try:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '--', sys.executable, os.path.abspath(__file__),
               '--kernel-pass', '--batch', str(args.batch), '--kernel-calls', str(args.kernel_calls)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        if r.returncode != 0:
            raise RuntimeError('the rocprofv3 pass failed (%d):\n%s' % (r.returncode, r.stdout.decode()[-3000:]))
        durs = {}
        for row in rows_of(tmp, 'kernel_trace.csv'):
            durs.setdefault(row['Kernel_Name'], []).append(int(row['End_Timestamp']) - int(row['Start_Timestamp']))
        if args.stats_out:
            stats(tmp, args.stats_out, 'rocprofv3 --kernel-trace --stats -- python tools/bench_repose.py --kernel-pass --batch %d '
                  '--kernel-calls %d (MI355X; S = 128, K = 10, bf16; %d photos of about 512 x 384 with one box of about 250 x 250 each; every '
                  'launch of %d repose calls, warm-up and graph capture included)' % (args.batch, args.kernel_calls, args.batch,
                                                                                    args.kernel_calls + 2))
        return durs
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(args):
    if args.kernel_pass:
        return kernel_pass(args)
    # the profiled pass first, in its own process, before this one opens the GPU
    durs = {} if args.no_profile else profile_kernels(args)
    import torch
    from bench_detect import timed_ms
    from imm_amd.inference import pack_u8, plan_buckets, stage_u8
    from imm_amd.keypoints import check_boxes
    B = args.batch
    photos, boxes, lm = scene(B)
    model, gen = make_generator(B)
    assert len(plan_buckets(B, B)) == 1
    props = torch.cuda.get_device_properties(0)
    lm_d = torch.from_numpy(lm).cuda()
    crops = torch.empty(B, S, S, 3, device='cuda:0')                # the same boxes cut and resized beforehand (imm_resize_crop_u8)
    rows = check_boxes(boxes, B)
    stage_u8(photos, crops, S, 'cuda:0', boxes=rows)
    torch.cuda.synchronize()
    # same faces either way: the timing compares like with like
    out, faces, _ = gen.repose(photos, lm_d, boxes, return_faces=True)
    same = bool(torch.equal(faces, gen.render(crops, lm_d)))
    fns = {'repose': lambda: gen.repose(photos, lm_d, boxes), 'render': lambda: gen.render(crops, lm_d),
           'pack': lambda: pack_u8(photos, 'cuda:0', rows)[0].clone()}
    ms = {k: [] for k in fns}
    for k, fn in fns.items():
        timed_ms(fn, 2, 1, args.warmup)
    for _ in range(args.windows):                                   # alternated: one window of each, again and again
        for k, fn in fns.items():
            ms[k].append(timed_ms(fn, args.reps, 1, 0))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in ms.items()}
    photo_b, face_b = compose_bytes(photos, boxes)
    lines = ['device: %s (%s, %d CUs)' % (props.name, props.gcnArchName, props.multi_processor_count),
             'S = %d, K = %d, bf16, one bucket of B = %d rows; %d u8 photos of about 512 x 384 (%.1f MB packed), one box of about 250 x 250 '
             'each; ms per call: median (min .. max) of %d alternated windows x %d calls' % (
                 S, K, B, B, sum(p.size for p in photos) / 1e6, args.windows, args.reps),
             'faces of repose == render on the pre-cropped tensors, bit for bit: %s' % same,
             '%-8s %10s %22s %12s' % ('call', 'ms', '(min .. max)', 'faces/s')]
    for k in ('repose', 'render', 'pack'):
        lines.append('%-8s %10.3f %22s %12s' % (k, med[k], '(%.3f .. %.3f)' % spread[k], '-' if k == 'pack' else '%.0f' % (B / med[k] * 1e3)))
    lines.append('repose - render (packing and copying the photos, the device copy, box crop, compose): %.3f ms per call, %.1f us per face; '
                 'of it %.3f ms is pack' % (med['repose'] - med['render'], (med['repose'] - med['render']) / B * 1e3, med['pack']))
    row = {'batch': B, 'repose_ms': med['repose'], 'render_ms': med['render'], 'pack_ms': med['pack'], 'faces_equal': same}
    if args.no_profile:
        lines.append('compose kernel time: not measured (--no-profile)')
    else:
        name = [k for k in durs if 'compose_u8_kernel' in k]
        if len(name) != 1:
            raise RuntimeError('the kernel trace holds %d compose kernels: %s' % (len(name), sorted(durs)[:20]))
        d = np.array(durs[name[0]], dtype=np.float64)
        mean_us = float(d.mean()) / 1e3
        gbs = (photo_b + face_b) / d.mean()                        # bytes per ns = GB/s
        lines += ['compose_u8_kernel (rocprofv3 --kernel-trace --stats, a run of its own): %d launches, mean %.1f us (min %.1f, max %.1f)' % (
                      len(d), mean_us, d.min() / 1e3, d.max() / 1e3),
                  'algorithmic bytes per launch: %.2f MB of photo pixels (3 read + 3 written per box pixel) + %.2f MB of faces (3 f32 channels; '
                  'the prediction buffer\'s pixel stride is %d) = %.2f MB' % (photo_b / 1e6, face_b / 1e6, gen.ldp, (photo_b + face_b) / 1e6),
                  'achieved %.0f GB/s = %.1f %% of the measured HBM copy rate (%.2f TB/s; %.0f TB/s specified)' % (
                      gbs, 100.0 * gbs / (HBM_MEASURED_TBS * 1e3), HBM_MEASURED_TBS, HBM_SPEC_TBS)]
        row.update(compose_us=mean_us, compose_bytes=photo_b + face_b, compose_gbs=gbs)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    print(json.dumps(row))


if __name__ == '__main__':
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--windows', type=int, default=7)
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--kernel-calls', type=int, default=10, help='repose calls of the profiled pass')
    p.add_argument('--no-profile', action='store_true', help='skip the rocprofv3 pass')
    p.add_argument('--kernel-pass', action='store_true', help='(internal) the workload of the profiled pass')
    p.add_argument('--out', type=str, default=OUT)
    p.add_argument('--stats-out', type=str, default=STATS)
    main(p.parse_args())
