"""Images/s of landmark detection: LandmarkDetector.detect (pose encoder only, batch norm folded, one captured program per batch
bucket) against the existing eval path, IMMModel.build(training_pl=False, build_loss=False) (both encoders and the renderer with
batch norm in eval mode), at S = 128, K = 10, bf16 and B in {32, 100, 256}.

Columns per batch B (median over windows of HIP-event-timed calls on the caller's stream, after warm-up):
  detect        detector.detect(images) on a resident device batch: input copy + graph replay + result copy, as a user calls it
  detect_graph  the detector's captured program alone (graph replay)
  eval_build    model.build(inputs, training_pl=False, build_loss=False): the engine's eager launch program, as eval runs today
  eval_graph    the same forward program (IMMEngine.forward_model_only) captured once and replayed: its best case
Usage: python tools/bench_detect.py [--batches 32 100 256] [--windows 7] [--reps 10]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imm_amd import ops                                   # noqa: E402
from imm_amd.models.imm_model import IMMModel             # noqa: E402
from imm_amd.utils.box import Box                         # noqa: E402


def model_config(n_maps):
    """configs/experiments/celeba-10pts.yaml `model:` block, synthetic perceptual network (bench.py's)."""
    return Box(dict(gauss_std=0.10, gauss_mode='rot', n_maps=n_maps, n_filters=32, block_sizes=[1, 1, 1],
                    n_filters_render=32, renderer_stride=2, min_res=16, same_n_filt=False,
                    reconstruction_loss='perceptual',
                    perceptual=dict(l2=True, comp=['input', 'conv1_2', 'conv2_2', 'conv3_2', 'conv4_2', 'conv5_2'],
                                    net_file='synthetic'),
                    loss_mask=True, confidence=False, channels_bug_fix=True))


def timed_ms(fn, reps, windows, warmup):
    """Median over `windows` of the mean per-call time (ms) of `reps` back-to-back calls, HIP events on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    out.sort()
    return out[len(out) // 2]


def main(args):
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    S, K = 128, 10
    rows = []
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        images = ops.to_device_pinned(torch.rand(B, S, S, 3, generator=g) * 255.0, dev)
        model = IMMModel(model_config(K), dtype=torch.bfloat16, device=dev)
        inputs = {'image': images, 'future_image': images}
        model.build(inputs, training_pl=False, build_loss=False)          # creates the batch-B engine (the variables)
        eng = model.engine
        det = model.landmark_detector(S, max_batch=B)
        row = {'batch': B}
        row['detect'] = timed_ms(lambda: det.detect(images), args.reps, args.windows, args.warmup)

        def det_graph():
            det.stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(det.stream):
                det._run(B)
            torch.cuda.current_stream().wait_stream(det.stream)
        row['detect_graph'] = timed_ms(det_graph, args.reps, args.windows, args.warmup)
        row['eval_build'] = timed_ms(lambda: model.build(inputs, training_pl=False, build_loss=False), args.reps, args.windows,
                                     args.warmup)
        # the eval forward program captured once (inputs are already in the engine's buffers)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.forward_model_only(False)
            side.synchronize()
            graph = ops.Graph()
            graph.capture_begin()
            eng.forward_model_only(False)
            graph.capture_end()
        side.synchronize()

        def eval_graph():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                graph.launch()
            torch.cuda.current_stream().wait_stream(side)
        row['eval_graph'] = timed_ms(eval_graph, args.reps, args.windows, args.warmup)
        # the two paths compute the same landmarks (the detector's parity tests bound this at 1e-3)
        mu_det = det.detect(images)
        model.build(inputs, training_pl=False, build_loss=False)
        row['max_abs_dmu'] = float((mu_det - eng.mu).abs().max())
        for k in ('detect', 'detect_graph', 'eval_build', 'eval_graph'):
            row[k + '_images_per_s'] = B / row[k] * 1e3
        row['speedup_vs_eval_build'] = row['eval_build'] / row['detect']
        row['speedup_vs_eval_graph'] = row['eval_graph'] / row['detect']
        print('B %3d  detect %.3f ms (%.0f img/s, graph alone %.3f ms)  eval build %.3f ms (%.0f img/s)  eval graph %.3f ms '
              '(%.0f img/s)  speed-up %.2fx vs build, %.2fx vs eval graph  max|dmu| %.2e' % (
                  B, row['detect'], row['detect_images_per_s'], row['detect_graph'], row['eval_build'],
                  row['eval_build_images_per_s'], row['eval_graph'], row['eval_graph_images_per_s'], row['speedup_vs_eval_build'],
                  row['speedup_vs_eval_graph'], row['max_abs_dmu']), flush=True)
        rows.append(row)
        del det, graph, eng, model
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    print(json.dumps({'image_size': S, 'n_maps': K, 'dtype': 'bf16', 'windows': args.windows, 'reps': args.reps, 'rows': rows}))


if __name__ == '__main__':
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--batches', type=int, nargs='+', default=[32, 100, 256])
    p.add_argument('--windows', type=int, default=7)
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    main(p.parse_args())
