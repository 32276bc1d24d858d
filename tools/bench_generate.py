"""Images/s of image generation: ImageGenerator.reconstruct (both encoders and the renderer, batch norm folded, captured programs
per batch bucket) against the existing eval path, IMMModel.build(training_pl=False, build_loss=False)['future_im_pred'], at
S = 128, K = 10, bf16 and B in {32, 128, 256}.

Columns per batch B (median over windows of HIP-event-timed calls on the caller's stream, after warm-up):
  reconstruct   gen.reconstruct(x, y) on resident device batches: copies in, the three stages' graphs, copies out, as a user calls it
  appearance / pose / render   each stage's captured program alone (graph replay at bucket B)
  upsample share   the imm_upsample2x_fwd launches' share of the render program, from its launches timed one by one (eager)
  eval_build    model.build(inputs, training_pl=False, build_loss=False): the engine's eager launch program, as eval runs today
  eval_graph    the same forward program (IMMEngine.forward_model_only) captured once and replayed (tools/bench_detect.py's way)
Usage: python tools/bench_generate.py [--batches 32 128 256] [--windows 7] [--reps 10]"""
import argparse
import json
import os
import socket
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from imm_amd import ops                                   # noqa: E402
from imm_amd.models.imm_model import IMMModel             # noqa: E402
from bench_detect import model_config, timed_ms           # noqa: E402


def on_stream(stream, fn):
    def run():
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            fn()
        torch.cuda.current_stream().wait_stream(stream)
    return run


def launch_times(prog, reps):
    """Per-launch time (ms) of a program's launches issued one by one, each timed over `reps` back-to-back calls."""
    out = []
    for l in prog:
        for _ in range(2):
            l.fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            l.fn()
        e1.record()
        e1.synchronize()
        out.append((l.tag, e0.elapsed_time(e1) / reps))
    return out


def main(args):
    torch.cuda.set_device(0)
    dev = 'cuda:0'
    S, K = 128, 10
    rows = []
    props = torch.cuda.get_device_properties(0)
    box = {'host': socket.gethostname(), 'device': props.name, 'gcn_arch': getattr(props, 'gcnArchName', ''),
           'uuid': str(getattr(props, 'uuid', '')), 'pci_bus_id': getattr(props, 'pci_bus_id', None),
           'date': time.strftime('%Y-%m-%d %H:%M:%S %Z')}
    print('# box %s' % json.dumps(box), flush=True)
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        x = ops.to_device_pinned(torch.rand(B, S, S, 3, generator=g) * 255.0, dev)
        y = ops.to_device_pinned(torch.rand(B, S, S, 3, generator=g) * 255.0, dev)
        model = IMMModel(model_config(K), dtype=torch.bfloat16, device=dev)
        inputs = {'image': x, 'future_image': y}
        model.build(inputs, training_pl=False, build_loss=False)          # creates the batch-B engine (the variables)
        eng = model.engine
        gen = model.image_generator(S, max_batch=B)
        row = {'batch': B}
        row['reconstruct'] = timed_ms(lambda: gen.reconstruct(x, y), args.reps, args.windows, args.warmup)
        row['appearance'] = timed_ms(on_stream(gen.stream, lambda: gen._run('appearance', B)), args.reps, args.windows, args.warmup)
        row['pose'] = timed_ms(on_stream(gen.detector.stream, lambda: gen.detector._run(B)), args.reps, args.windows, args.warmup)
        row['render'] = timed_ms(on_stream(gen.stream, lambda: gen._run('render', B)), args.reps, args.windows, args.warmup)
        with torch.cuda.stream(gen.stream):
            lt = launch_times(gen.program('render', B), args.reps)
        gen.stream.synchronize()
        row['render_launches_ms'] = sum(t for _tag, t in lt)
        row['upsample_ms'] = sum(t for tag, t in lt if tag == 'upsample')
        row['upsample_share_of_render'] = row['upsample_ms'] / row['render_launches_ms']
        row['eval_build'] = timed_ms(lambda: model.build(inputs, training_pl=False, build_loss=False), args.reps, args.windows,
                                     args.warmup)
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
        row['eval_graph'] = timed_ms(on_stream(side, graph.launch), args.reps, args.windows, args.warmup)
        # the two paths compute the same image (the generator's parity tests bound this against the oracle)
        pred = gen.reconstruct(x, y)
        _, _, _, t = model.build(inputs, training_pl=False, output_tensors=True, build_loss=False)
        ref = t['future_im_pred']
        row['rel_l2_vs_eval'] = float((pred - ref).norm() / ref.norm())
        for k in ('reconstruct', 'eval_build', 'eval_graph'):
            row[k + '_images_per_s'] = B / row[k] * 1e3
        row['speedup_vs_eval_build'] = row['eval_build'] / row['reconstruct']
        row['speedup_vs_eval_graph'] = row['eval_graph'] / row['reconstruct']
        print('B %3d  reconstruct %.3f ms (%.0f img/s; appearance %.3f  pose %.3f  render %.3f ms, up-sampling %.1f %% of the '
              'render launches)  eval build %.3f ms (%.0f img/s)  eval graph %.3f ms (%.0f img/s)  speed-up %.2fx vs build, '
              '%.2fx vs eval graph  rel L2 vs eval %.2e' % (
                  B, row['reconstruct'], row['reconstruct_images_per_s'], row['appearance'], row['pose'], row['render'],
                  100 * row['upsample_share_of_render'], row['eval_build'], row['eval_build_images_per_s'], row['eval_graph'],
                  row['eval_graph_images_per_s'], row['speedup_vs_eval_build'], row['speedup_vs_eval_graph'],
                  row['rel_l2_vs_eval']), flush=True)
        rows.append(row)
        del gen, graph, eng, model
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    print(json.dumps({'image_size': S, 'n_maps': K, 'dtype': 'bf16', 'windows': args.windows, 'reps': args.reps, 'box': box, 'rows': rows}))


if __name__ == '__main__':
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--batches', type=int, nargs='+', default=[32, 128, 256])
    p.add_argument('--windows', type=int, default=7)
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    main(p.parse_args())
