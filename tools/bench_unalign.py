"""Faces/s of ImageGenerator.repose with a template (align -> encode -> render -> paste through the inverse map) against repose with
raw box crops on the same photos, and of LandmarkDetector.unalign on pre-aligned device faces, at S = 128, bf16, K = 10 and one bucket
of B = 64 rows; the scene is tools/bench_repose.py's (photos of about 512 x 384, one box of about 250 x 250 each).  Writes the table
to profiles/unalign_bench.txt and the kernel times to profiles/unalign_kernel_stats.csv.

  repose_tpl   gen.repose(photos, landmarks, boxes, template=tpl): the photos packed once, the detector's align program and warp, the
               appearance and render graphs, imm_unalign_maps once and one imm_unalign_u8 launch
  repose       gen.repose(photos, landmarks, boxes): the box-crop path (tools/bench_repose.py measures it on its own)
  unalign      det.unalign(photos, faces, alignment) on faces and coefficients that are already on the device: the photos packed,
               imm_unalign_maps, one imm_unalign_u8 launch.  The alignment is SYNTHETIC: similarity maps about each box's centre, turned
               by up to 25 degrees either way and scaled by 0.9 to 1.1, so that an aligned face covers about its box
  align        det.align(photos, tpl, boxes, return_transform=True): what repose_tpl runs ahead of the generator
  pack         inference.pack_u8 of the photos: the host-side part of every call above
All are timed with HIP events on the caller's stream, alternated window by window in the same run (median over the windows of the mean
per-call time).  The model is untrained and the photos are noise: its landmarks nearly coincide, so the maps that repose_tpl fits to a
spread-out template shrink every aligned frame to a few photo pixels.  Its end-to-end time stands (the host work and the programs do not
depend on the maps), but its paste covers next to nothing; the number of photo pixels each set of maps covers is counted and printed.

The kernels' own times therefore come from the synthetic maps, in a second process: `rocprofv3 --kernel-trace --stats -- python
tools/bench_unalign.py --kernel-pass` runs det.unalign calls only (a run of its own: tracing slows the host, so no end-to-end number is
taken from it).  The paste's algorithmic bytes are counted from the maps: 6 per covered photo pixel (3 read, 3 written) plus the three
channels of every face once (S * S * 12); the rate is those bytes over the kernel's mean time, set against the 6.29 TB/s a float4 copy
measures on this part (8 TB/s specified).
Usage: python tools/bench_unalign.py [--batch 64] [--windows 7] [--reps 10]"""
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

from bench_repose import HBM_MEASURED_TBS, HBM_SPEC_TBS, K, S, make_generator, scene      # noqa: E402

OUT = os.path.join(ROOT, 'profiles', 'unalign_bench.txt')
STATS = os.path.join(ROOT, 'profiles', 'unalign_kernel_stats.csv')


def spread_template():
    """K well-separated template points on a spiral."""
    from imm_amd.alignment import LandmarkTemplate
    k = np.arange(K, dtype=np.float64)
    return LandmarkTemplate(np.stack([np.cos(2.4 * k), np.sin(2.4 * k)], axis=1) * (0.2 + 0.4 * k / K)[:, None], S)


def synthetic_alignment(boxes, tpl, seed=1):
    """An Alignment of similarity maps about each box's centre: rotation within 25 degrees either way, scale 0.9 to 1.1, a small shift."""
    from imm_amd import ops
    from imm_amd.alignment import Alignment
    from imm_amd.keypoints import box_geometry, check_boxes
    rng = np.random.RandomState(seed)
    rows = check_boxes(boxes, len(boxes))
    n = len(rows)
    a = rng.uniform(0.9, 1.1, n) * np.exp(1j * np.deg2rad(rng.uniform(-25.0, 25.0, n)))
    b = rng.uniform(-0.05, 0.05, n) + 1j * rng.uniform(-0.05, 0.05, n)
    # T(q) = a q + b with q = q_y + i q_x: rows 1, q_y, q_x of (y, x) coefficients (LandmarkTemplate.fit_matrix)
    coef = np.stack([np.stack([b.real, b.imag], 1), np.stack([a.real, a.imag], 1), np.stack([-a.imag, a.real], 1)], axis=1).astype(np.float32)
    return Alignment(ops.to_device_pinned(coef, 'cuda:0'), ops.to_device_pinned(box_geometry(rows, S), 'cuda:0'), None, 'similarity', 0.0,
                     tpl, S, rows)


def covered_pixels(fwd, bbox, So):
    """Photo pixels the paste touches: per row the pixels of its bbox whose aligned coordinate lies in [0, So - 1]^2 (f32, the
    kernel's operation order)."""
    f32 = np.float32
    total = 0
    for m, (y0, x0, y1, x1) in zip(np.asarray(fwd, dtype=f32), np.asarray(bbox).tolist()):
        if y1 <= y0 or x1 <= x0 or not np.isfinite(m).all():
            continue
        r, c = np.arange(y0, y1, dtype=f32)[:, None], np.arange(x0, x1, dtype=f32)[None, :]
        fi = (m[0] * r + m[1] * c) + m[2]
        fj = (m[3] * r + m[4] * c) + m[5]
        total += int(((fi >= 0) & (fi <= So - 1) & (fj >= 0) & (fj <= So - 1)).sum())
    return total


def maps_of(photos, al):
    """(fwd, bbox) of an alignment over these photos, from imm_unalign_maps, as host arrays."""
    import torch
    from imm_amd import ops
    from imm_amd.inference import pack_u8
    _src, _offs, hw_d, boxes_d = pack_u8(photos, 'cuda:0', al.rows)
    n = len(al.rows)
    fwd = torch.empty(n, 6, device='cuda:0')
    bbox = torch.empty(n, 4, dtype=torch.int32, device='cuda:0')
    ops.unalign_maps(al.coef, al.geom, boxes_d, hw_d, S, al.out_size, fwd, bbox)
    torch.cuda.synchronize()
    return fwd.cpu().numpy(), bbox.cpu().numpy()


def kernel_pass(args):
    """What the profiled child runs: a few det.unalign calls over the synthetic maps, nothing timed; the covered pixel count goes to
    --pass-out."""
    import torch
    photos, boxes, _lm = scene(args.batch)
    _model, gen = make_generator(args.batch)
    al = synthetic_alignment(boxes, spread_template())
    faces = torch.rand(args.batch, S, S, 3, device='cuda:0') * 255.0
    for _ in range(args.kernel_calls + 2):
        gen.detector.unalign(photos, faces, al)
    torch.cuda.synchronize()
    fwd, bbox = maps_of(photos, al)
    if args.pass_out:
        with open(args.pass_out, 'w') as f:
            json.dump({'covered': covered_pixels(fwd, bbox, S), 'bbox_pixels': int(((bbox[:, 2] - bbox[:, 0]) * (bbox[:, 3] - bbox[:, 1])).sum())}, f)


def profile_kernels(args):
    """Run the kernel pass under rocprofv3 in a process of its own; returns ({kernel name: [durations ns]}, the pass's counts)."""
    from profile_summary import rows_of, stats
    tmp = tempfile.mkdtemp(prefix='unalign_prof_')
    try:
        pass_out = os.path.join(tmp, 'pass.json')
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '--', sys.executable, os.path.abspath(__file__),
               '--kernel-pass', '--batch', str(args.batch), '--kernel-calls', str(args.kernel_calls), '--pass-out', pass_out]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        if r.returncode != 0:
            raise RuntimeError('the rocprofv3 pass failed (%d):\n%s' % (r.returncode, r.stdout.decode()[-3000:]))
        durs = {}
        for row in rows_of(tmp, 'kernel_trace.csv'):
            durs.setdefault(row['Kernel_Name'], []).append(int(row['End_Timestamp']) - int(row['Start_Timestamp']))
        if args.stats_out:
            stats(tmp, args.stats_out, 'rocprofv3 --kernel-trace --stats -- python tools/bench_unalign.py --kernel-pass --batch %d '
                  '--kernel-calls %d (MI355X; S = 128, K = 10, bf16; %d photos of about 512 x 384 with one box of about 250 x 250 each; every '
                  'launch of %d det.unalign calls over synthetic similarity maps)' % (
                      args.batch, args.kernel_calls, args.batch, args.kernel_calls + 2))
        with open(pass_out) as f:
            return durs, json.load(f)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def one_kernel(durs, name):
    found = [k for k in durs if name in k]
    if len(found) != 1:
        raise RuntimeError('the kernel trace holds %d kernels named %s: %s' % (len(found), name, sorted(durs)[:20]))
    return np.array(durs[found[0]], dtype=np.float64)


def main(args):
    if args.kernel_pass:
        return kernel_pass(args)
    # the profiled pass first, in its own process, before this one opens the GPU
    durs, counts = ({}, {}) if args.no_profile else profile_kernels(args)
    import torch
    from bench_detect import timed_ms
    from imm_amd.inference import pack_u8, plan_buckets
    from imm_amd.keypoints import check_boxes
    B = args.batch
    photos, boxes, lm = scene(B)
    model, gen = make_generator(B)
    det = gen.detector
    assert len(plan_buckets(B, B)) == 1
    props = torch.cuda.get_device_properties(0)
    lm_d = torch.from_numpy(lm).cuda()
    rows = check_boxes(boxes, B)
    tpl = spread_template()
    _aligned, al_model = det.align(photos, tpl, boxes, return_transform=True)
    covered_model = covered_pixels(*maps_of(photos, al_model), S)
    al = synthetic_alignment(boxes, tpl)
    faces = torch.rand(B, S, S, 3, device='cuda:0') * 255.0
    fwd, bbox = maps_of(photos, al)
    covered = covered_pixels(fwd, bbox, S)
    # the same call twice gives the same bytes: the timing repeats one computation
    a = [o.clone() for o in gen.repose(photos, lm_d, boxes, template=tpl)]
    same = all(bool(torch.equal(x, y)) for x, y in zip(a, gen.repose(photos, lm_d, boxes, template=tpl)))
    fns = {'repose_tpl': lambda: gen.repose(photos, lm_d, boxes, template=tpl), 'repose': lambda: gen.repose(photos, lm_d, boxes),
           'unalign': lambda: det.unalign(photos, faces, al), 'align': lambda: det.align(photos, tpl, boxes, return_transform=True),
           'pack': lambda: pack_u8(photos, 'cuda:0', rows)[0]}
    ms = {k: [] for k in fns}
    for k, fn in fns.items():
        timed_ms(fn, 2, 1, args.warmup)
    for _ in range(args.windows):                                   # alternated: one window of each, again and again
        for k, fn in fns.items():
            ms[k].append(timed_ms(fn, args.reps, 1, 0))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in ms.items()}
    box_px = int(((rows[:, 3] - rows[:, 1]) * (rows[:, 4] - rows[:, 2])).sum())
    face_b = B * S * S * 3 * 4
    lines = ['device: %s (%s, %d CUs)' % (props.name, props.gcnArchName, props.multi_processor_count),
             'S = %d, K = %d, bf16, one bucket of B = %d rows; %d u8 photos of about 512 x 384 (%.1f MB packed), one box of about 250 x 250 '
             'each; ms per call: median (min .. max) of %d alternated windows x %d calls' % (
                 S, K, B, B, sum(p.size for p in photos) / 1e6, args.windows, args.reps),
             'photo pixels the synthetic maps of unalign cover: %d (%.2f of the %d box pixels); their bounding boxes: %d pixels' % (
                 covered, covered / float(box_px), box_px, int(((bbox[:, 2] - bbox[:, 0]) * (bbox[:, 3] - bbox[:, 1])).sum())),
             'photo pixels the maps of repose_tpl cover (an untrained model\'s landmarks against a spread-out template): %d' % covered_model,
             'repose(template=) twice, the same bytes: %s' % same,
             '%-11s %10s %22s %12s' % ('call', 'ms', '(min .. max)', 'faces/s')]
    for k in ('repose_tpl', 'repose', 'unalign', 'align', 'pack'):
        lines.append('%-11s %10.3f %22s %12s' % (k, med[k], '(%.3f .. %.3f)' % spread[k], '-' if k == 'pack' else '%.0f' % (B / med[k] * 1e3)))
    lines.append('repose_tpl - repose (the detector\'s align program and warp in place of the box crop, the paste in place of compose): '
                 '%.3f ms per call, %.1f us per face' % (med['repose_tpl'] - med['repose'], (med['repose_tpl'] - med['repose']) / B * 1e3))
    row = {'batch': B, 'repose_template_ms': med['repose_tpl'], 'repose_ms': med['repose'], 'unalign_ms': med['unalign'],
           'align_ms': med['align'], 'pack_ms': med['pack'], 'covered_pixels': covered, 'covered_pixels_repose_template': covered_model,
           'repeatable': same}
    if args.no_profile:
        lines.append('kernel times: not measured (--no-profile)')
    else:
        d, dm = one_kernel(durs, 'unalign_u8_kernel'), one_kernel(durs, 'unalign_maps_kernel')
        photo_b = 6 * int(counts['covered'])
        gbs = (photo_b + face_b) / d.mean()                        # bytes per ns = GB/s
        lines += ['unalign_u8_kernel (rocprofv3 --kernel-trace --stats, a run of its own): %d launches, mean %.1f us (min %.1f, max %.1f) = '
                  '%.2f %% of a repose_tpl call, %.2f %% of an unalign call' % (
                      len(d), d.mean() / 1e3, d.min() / 1e3, d.max() / 1e3, 100.0 * d.mean() / 1e6 / med['repose_tpl'],
                      100.0 * d.mean() / 1e6 / med['unalign']),
                  'unalign_maps_kernel: %d launches, mean %.1f us (min %.1f, max %.1f)' % (len(dm), dm.mean() / 1e3, dm.min() / 1e3, dm.max() / 1e3),
                  'algorithmic bytes per paste launch: %.2f MB of photo pixels (3 read + 3 written per covered pixel, %d of them) + %.2f MB of '
                  'faces (3 f32 channels, pixel stride 3) = %.2f MB' % (
                      photo_b / 1e6, int(counts['covered']), face_b / 1e6, (photo_b + face_b) / 1e6),
                  'achieved %.0f GB/s = %.1f %% of the measured HBM copy rate (%.2f TB/s; %.0f TB/s specified); imm_compose_u8 reaches 16 %% '
                  '(profiles/repose_bench.txt)' % (gbs, 100.0 * gbs / (HBM_MEASURED_TBS * 1e3), HBM_MEASURED_TBS, HBM_SPEC_TBS)]
        row.update(unalign_u8_us=d.mean() / 1e3, unalign_maps_us=dm.mean() / 1e3, unalign_bytes=photo_b + face_b, unalign_gbs=gbs)
    lines.append('not measured: other photo and face sizes, several faces per photo (the link walks), the affine model, out_size != S, the paste at '
                 'the prediction buffer\'s pixel stride with maps of a trained model')
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
    p.add_argument('--kernel-calls', type=int, default=10, help='repose(template=) calls of the profiled pass')
    p.add_argument('--no-profile', action='store_true', help='skip the rocprofv3 pass')
    p.add_argument('--kernel-pass', action='store_true', help='(internal) the workload of the profiled pass')
    p.add_argument('--pass-out', type=str, default=None, help='(internal) where the profiled pass writes its pixel counts')
    p.add_argument('--out', type=str, default=OUT)
    p.add_argument('--stats-out', type=str, default=STATS)
    main(p.parse_args())
