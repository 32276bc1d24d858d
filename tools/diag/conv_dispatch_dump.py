"""Dump what the library answers about kernel dispatch for a grid of convolution descriptors, one line per descriptor: run it
against two builds (IMM_HIP_LIB=<other .so>) and diff the outputs — a refactor of the host-side dispatch leaves 0 lines.

    python tools/diag/conv_dispatch_dump.py [--programs] > dump.txt

Queries only (no launch): it runs without a GPU (the library then plans for 256 CUs).  IMM_CONV_DISABLE in the
environment selects the fallback dispatch.  --programs (needs a GPU) adds the (name, tag, variant) list of the benchmark engine's
forward and backward programs.  The last lines count the descriptors per kernel family and the positive answers per
"supported" query; the script fails when one of them is 0 (the sweep would prove nothing about that family)."""
import argparse
import ctypes as C
import itertools
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from imm_amd import _lib as L, ops  # noqa: E402

FLAG_SETS = [('none', 0), ('bias+relu', L.CONV_BIAS | L.CONV_RELU), ('bias+stats', L.CONV_BIAS | L.CONV_STATS), ('mask', L.CONV_MASK),
             ('mask+stats', L.CONV_MASK | L.CONV_STATS), ('f32', L.CONV_OUT_F32)]
DTYPES = [('bf16', torch.bfloat16), ('f16', torch.float16), ('f32', torch.float32)]
SIDES = (8, 16, 32, 64, 128)
CHANNELS = (16, 32, 64, 128, 256, 512)


def descs():
    """(label, ConvDesc): batch x side x ci x co x k x stride x updiv x flags, co = 20 and the 7x1 first layer included."""
    for batch, side, ci, co, k, stride, updiv, (fname, flags) in itertools.product(
            (1, 2, 8, 32), SIDES, CHANNELS, CHANNELS + (20,), (1, 3), (1, 2), (1, 2), FLAG_SETS):
        ld = ops.round_up(co, 8)
        if updiv == 1:
            d = ops.fwd_desc(batch, side, side, ci, ci, co, ld, k, stride, flags, ldmask=ld)
        else:           # the data gradient of a stride-2 convolution (ci channels of dy -> co channels of dx at twice the side)
            d = ops.dgrad_desc(batch, 2 * side, 2 * side, co, ld, ci, ci, k, 2, flags, ldmask=ld)
            d.stride = stride
        yield 'b%d s%d ci%d co%d k%d st%d up%d %s' % (batch, side, ci, co, k, stride, updiv, fname), d
    for batch, side, (fname, flags) in itertools.product((1, 2, 8, 32), SIDES, FLAG_SETS):
        yield 'b%d s%d 7x1 %s' % (batch, side, fname), ops.fwd_desc(batch, side, side, 32, 32, 32, 32, 7, 1, flags, ldmask=32, kw=1)


def quiet(fn, *a):
    try:
        return fn(*a)
    except L.ImmHipError:
        return 'err'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--programs', action='store_true')
    args = ap.parse_args()
    lib = L.load()
    families, positives = {f: 0 for f in range(1, 9)}, {'tap': 0, 'dgrad_s2': 0}
    out = []
    for label, d in descs():
        lddy = ops.round_up(d.co, 8)
        cols = []
        for dname, dt in DTYPES:
            fam, key = quiet(ops.conv2d_variant, d, dt), None
            if fam != 'err':
                fam, key = fam
                families[key // 100000] += 1
            cols.append('%s:%s/%s' % (dname, key, ','.join(str(v) for v in ops.conv2d_wgrad_variant(d, lddy, dt))))
        tap = int(ops.conv2d_tap_supported(d))
        positives['tap'] += tap
        out.append('%s | %s | rows %s ws %d splits %s tap %d' % (
            label, ' '.join(cols), quiet(ops.conv_stats_blocks, d), lib.imm_conv2d_workspace_bytes(C.byref(d)),
            quiet(ops.conv2d_wgrad_splits, d, lddy), tap))
    # the one-launch stride-2 data gradient and the four-class group it replaces
    for batch, side, ci, co, (fname, flags) in itertools.product((1, 2, 8, 32), SIDES, CHANNELS, CHANNELS + (20,), (FLAG_SETS[0], FLAG_SETS[4])):
        ld = ops.round_up(co, 8)
        s2 = int(ops.conv2d_dgrad_s2_supported(batch, side, side, ci, co, ld))
        positives['dgrad_s2'] += s2
        classes = ops.dgrad_s2_class_descs(batch, 2 * side, 2 * side, co, ld, ci, ci, 3, flags, ldmask=ld)
        group = types.SimpleNamespace(descs=(L.ConvDesc * 4)(*[c for c, _mode in classes]), n=4)
        out.append('b%d s%d ci%d co%d %s | dgrad_s2 %d group_rows %s' % (batch, side, ci, co, fname, s2, quiet(ops.conv2d_group_stats_blocks, group)))
    if args.programs:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
        import bench
        from imm_amd.models.imm_model import IMMModel
        from imm_amd.train.cnn_train_multi import TrainStep
        model = IMMModel(bench.model_config(bench.N_MAPS), dtype=torch.bfloat16, device='cuda:0')
        eng = TrainStep(model, bench.BATCH_PER_GPU, bench.IMAGE_SIZE, world_size=1, use_graph=False).engine
        for pname, prog in (('fwd', eng.prog_fwd), ('bwd', eng.prog_bwd)):
            out.extend('program %s | %s | %s | %s' % (pname, l.name, l.tag, l.variant) for l in prog)
    out.extend('count family %d: %d' % kv for kv in sorted(families.items()))
    out.extend('count %s supported: %d' % kv for kv in sorted(positives.items()))
    print('\n'.join(out))
    complete = all(families.values()) and all(positives.values())
    return 0 if complete or os.environ.get('IMM_CONV_DISABLE') else 1       # (a disabled family has no descriptor, by design)


if __name__ == '__main__':
    sys.exit(main())
