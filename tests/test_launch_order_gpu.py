"""The launch sequence of every public inference method, pinned: the names of the library entry points a call issues, in order, with
use_graph off, and with use_graph on for the call that captures and for the call that replays.  Seven box rows at max_batch = 4 are
one full bucket and one padded bucket; after every call the padded tail of the input buffer that was staged is all zero.
`python tests/test_launch_order_gpu.py` prints the lists of the checkout it runs in, run-length coded."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_reference as WR                                                  # noqa: E402
from alignment_reference import jittered_grid_template, smooth_photo         # noqa: E402
from test_generator_gpu import make_model as make_generator_model            # noqa: E402
from test_warp_gpu import S                                                  # noqa: E402

pytestmark = pytest.mark.gpu
K, MAX_BATCH = 10, 4
SIZES = ((96, 80), (64, 96), (72, 72))
ROWS = [(0, 4, 6, 70, 60), (1, -5, 10, 50, 90), (2, 0, 0, 72, 72), (0, 30, 20, 96, 80), (1, 8, 8, 40, 40), (2, 20, -6, 80, 50),
        (0, 10, 30, 60, 75)]
FACES = [(0, 4, 6, 70, 60), (0, 30, 20, 96, 80), (0, 10, 30, 60, 75)]        # the tracker's: three faces of frame 0
DRIVER = (4, 6, 70, 60)


def rle(names):
    """['a', 'b', 'b'] -> ['a', ('b', 2)]."""
    out = []
    for n in names:
        if out and out[-1][0] == n:
            out[-1][1] += 1
        else:
            out.append([n, 1])
    return [n if c == 1 else (n, c) for n, c in out]


class Recorder(object):
    """Every launch reaches the library through _lib.call, which ops binds by name: both names are wrapped, and restored on exit."""

    def __enter__(self):
        from imm_amd import _lib, ops
        self.names, self._mods, self._call = [], (_lib, ops), _lib.call
        assert ops.call is _lib.call

        def call(name, *args):
            self.names.append(name)
            return self._call(name, *args)
        for m in self._mods:
            m.call = call
        return self

    def __exit__(self, *exc):
        for m in self._mods:
            m.call = self._call


def cases():
    """name -> (fn(det, gen), [(object staged: 'det' | 'gen', count, bucket)]): the calls, and the padded buckets they leave.  A fourth
    entry before(det, gen) runs ahead of the recorder; what it returns is fn's third argument."""
    from imm_amd import alignment as AL
    from imm_amd.quality import QualityGate
    from imm_amd.keypoints import LandmarkRegressor
    from imm_amd.inference import plan_buckets
    assert plan_buckets(len(ROWS), MAX_BATCH) == [(0, 4, 4), (4, 3, 4)]
    rng = np.random.RandomState(4)
    ims = [smooth_photo(h, w, 70 + i) for i, (h, w) in enumerate(SIZES)]
    frames = [smooth_photo(96, 80, 80 + i) for i in range(3)]
    batch = torch.from_numpy(rng.uniform(0, 255, size=(7, S, S, 3)).astype(np.float32))
    whole = [smooth_photo(40 + 8 * i, 56 - 4 * i, 90 + i) for i in range(7)]
    _mu, poses = WR.landmarks(K, len(ROWS), rng)
    lm = torch.from_numpy(poses)
    reg = LandmarkRegressor(rng.standard_normal((10, 2 * K)) * 0.3, rng.standard_normal(10) * 5, K, S, True)
    tpl = AL.LandmarkTemplate(jittered_grid_template(K, 8), S)
    pad, gpad = [('det', 3, 4)], [('gen', 3, 4)]

    def unalign(det, gen):
        aligned, al = det.align(ims, tpl, ROWS, return_transform=True)
        return det.unalign(ims, aligned, al)
    return [
        ('detect_tensor', lambda det, gen: det.detect(batch), pad),
        ('detect_u8', lambda det, gen: det.detect(whole, heatmaps=True), pad),
        ('keypoints', lambda det, gen: det.keypoints(ims, reg, ROWS, return_mu=True), pad),
        ('landmarks', lambda det, gen: det.landmarks(ims, ROWS), pad),
        ('align_similarity', lambda det, gen: det.align(ims, tpl, ROWS), pad),
        ('align_tps', lambda det, gen: det.align(ims, tpl, ROWS, model='tps', out_size=64), pad),
        ('align_transform', lambda det, gen: det.align(ims, tpl, ROWS, model='affine', return_transform=True), pad),
        ('warp', lambda det, gen: det.warp(ims, poses, ROWS, return_transform=True), pad),
        ('morph', lambda det, gen: det.morph(ims, ims, ROWS, ROWS[::-1], shape=0.5, return_transform=True), pad),
        ('unalign', unalign, pad),
        ('render', lambda det, gen: gen.render(ims, lm, boxes=ROWS), gpad),
        ('transfer', lambda det, gen: gen.transfer(ims, ims, boxes=ROWS, pose_boxes=ROWS[:3]), pad + gpad),
        ('repose', lambda det, gen: gen.repose(ims, lm, ROWS, return_faces=True), gpad),
        ('repose_pose_photos', lambda det, gen: gen.repose(ims, ims[:1], ROWS, pose_boxes=ROWS[:1]), gpad),
        ('repose_template', lambda det, gen: gen.repose(ims, lm, ROWS, template=tpl), pad + gpad),
        ('track', lambda det, gen: det.track(frames, FACES, chunk_frames=2), pad),
        ('reenact', lambda det, gen: gen.reenact(ims, frames, DRIVER, ROWS[:3], return_faces=True), pad + gpad),
        # no pose program: nothing is staged
        ('redact', lambda det, gen: det.redact(ims, ROWS), []),
        ('redact_hull', lambda det, gen: det.redact(ims, ROWS, mode='smooth', mask='hull'), pad),
        ('annotate', lambda det, gen: det.annotate(ims, ROWS, draw=('points', 'box', 'hull', 'label')), pad),
        # three frames in chunks of two: a full chunk and a chunk of one frame; three faces and three donor rows: one padded bucket each
        ('morph_clip', lambda det, gen: det.morph_clip(frames, FACES, ims, ROWS[:3], chunk_frames=2), pad),
        ('morph_clip_full', lambda det, gen: det.morph_clip(frames, FACES, ims, ROWS[:3], colour=0.5, mask='hull', seamless=0.5,
                                                            colour_smooth=0.25, seam_smooth=0.5, chunk_frames=2), pad),
        ('redact_clip', lambda det, gen: det.redact_clip(frames, FACES, mask='hull', gate=QualityGate(0.5, 0.5), chunk_frames=2), pad),
        ('annotate_clip', lambda det, gen: det.annotate_clip(frames, FACES, draw=('points', 'box', 'hull'), trail=1, chunk_frames=2), pad),
        ('annotate_clip_track', lambda det, gen, tr: det.annotate_clip(frames, track=tr, draw=('points', 'box', 'hull'), trail=1,
                                                                       chunk_frames=2), [],
         lambda det, gen: det.track(frames, FACES, chunk_frames=2)),
    ]


def record(model):
    """{case: {'eager': [...], 'capture': [...], 'replay': [...]}} as flat lists of names; the padded tails are checked after every call."""
    from imm_amd.generation import ImageGenerator
    gens = {g: ImageGenerator(model, image_size=S, max_batch=MAX_BATCH, use_graph=g) for g in (False, True)}
    out = {}
    for name, fn, padded, *before in cases():
        out[name] = {}
        for mode in ('eager', 'capture', 'replay'):
            gen = gens[mode != 'eager']
            objs = {'det': gen.detector, 'gen': gen}
            made = [b(gen.detector, gen) for b in before]
            torch.cuda.synchronize()
            for x in objs.values():
                if mode == 'capture':
                    x._graphs = {}                     # the case's first call captures whatever it runs
                x._ensure_capacity(MAX_BATCH)
                x._img.fill_(1.0)
            with Recorder() as rec:
                fn(gen.detector, gen, *made)
            torch.cuda.synchronize()
            for who, count, bucket in padded:
                assert not objs[who]._img[count:bucket].any(), '%s (%s): the padded rows of %s._img are not zero' % (name, mode, who)
            out[name][mode] = list(rec.names)
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# What the parent of the bucket-runner refactor issued, recorded by this file's own recorder; the docstrings' "Per bucket: ..." sentences
# say the same.  ENC: a folded encoder; POSE: the detector's program; RENDER: the render stage; captured(p): a graph-cache miss (warm-up,
# capture, launch).
CROP, GO, COMPOSE, STEP, PASTE = 'imm_resize_crop_u8', 'imm_graph_launch', 'imm_compose_u8', 'imm_track_step', 'imm_unalign_u8'
ENC = ['imm_conv_first'] + ['imm_conv2d'] * 7
POSE = ENC + ['imm_pose_head_fwd']
ALIGN = POSE + ['imm_align_coeffs']
RENDER = ['imm_softargmax_gauss_fwd'] + (['imm_conv2d'] * 2 + ['imm_upsample2x_fwd']) * 3 + ['imm_conv2d'] * 2
WARP = ['imm_warp_fit', 'imm_warp_u8']
MORPH = ['imm_morph_poses', 'imm_warp_fit', 'imm_morph_u8']
FRAME = [STEP, 'imm_retarget']


def captured(p):
    return p + ['imm_graph_begin'] + p + ['imm_graph_end', GO]


def modes(eager, capture, replay):
    return {'eager': eager, 'capture': capture, 'replay': replay}


LANDMARKS = modes(([CROP] + POSE) * 2, [CROP] + captured(POSE) + [CROP, GO], [CROP, GO] * 2)
ALIGNED = modes(([CROP] + ALIGN + ['imm_align_warp_u8']) * 2,
                [CROP] + captured(ALIGN) + ['imm_align_warp_u8', CROP, GO, 'imm_align_warp_u8'], [CROP, GO, 'imm_align_warp_u8'] * 2)
EXPECTED = {
    'detect_tensor': modes(POSE * 2, captured(POSE) + [GO], [GO] * 2),
    'detect_u8': LANDMARKS,
    'keypoints': LANDMARKS,
    'landmarks': LANDMARKS,
    'align_similarity': ALIGNED,
    'align_tps': ALIGNED,
    'align_transform': ALIGNED,
    'warp': modes(([CROP] + POSE + WARP) * 2, [CROP] + captured(POSE) + WARP + [CROP, GO] + WARP, ([CROP, GO] + WARP) * 2),
    'morph': modes(LANDMARKS['eager'] + ([CROP] + POSE + MORPH) * 2, LANDMARKS['capture'] + ([CROP, GO] + MORPH) * 2,
                   LANDMARKS['replay'] + ([CROP, GO] + MORPH) * 2),
    'unalign': {m: ALIGNED[m] + ['imm_unalign_maps', PASTE] for m in ALIGNED},
    'render': modes(([CROP] + ENC + RENDER) * 2, [CROP] + captured(ENC) + captured(RENDER) + [CROP, GO, GO], [CROP, GO, GO] * 2),
    # the poses' three rows (one detector bucket), the seven appearance rows (two buckets), 21 pairs (five buckets of 4, one of 1)
    'transfer': modes([CROP] + POSE + ([CROP] + ENC) * 2 + RENDER * 6,
                      [CROP] + captured(POSE) + [CROP] + captured(ENC) + [CROP, GO] + captured(RENDER) + [GO] * 4 + captured(RENDER),
                      [CROP, GO] + [CROP, GO] * 2 + [GO] * 6),
    'repose': modes(([CROP] + ENC + RENDER + [COMPOSE]) * 2, [CROP] + captured(ENC) + captured(RENDER) + [COMPOSE, CROP, GO, GO, COMPOSE],
                    [CROP, GO, GO, COMPOSE] * 2),
    'repose_template': modes(ALIGNED['eager'] + ['imm_unalign_maps'] + (ENC + RENDER + [PASTE]) * 2,
                             ALIGNED['capture'] + ['imm_unalign_maps'] + captured(ENC) + captured(RENDER) + [PASTE, GO, GO, PASTE],
                             ALIGNED['replay'] + ['imm_unalign_maps'] + [GO, GO, PASTE] * 2),
    # the program is captured ahead of the first frame
    'track': modes(([CROP] + POSE + [STEP]) * 3, captured(POSE) + [CROP, GO, STEP] * 3, [CROP, GO, STEP] * 3),
    # once per call: the faces' landmarks, the render program captured ahead, the appearance stage; the tracker's program (bucket 1)
    'reenact': modes([CROP] + POSE + [CROP] + ENC + ([CROP] + POSE + FRAME + RENDER + [COMPOSE]) * 3,
                     [CROP] + captured(POSE) + [CROP] + captured(RENDER) + captured(ENC) + captured(POSE) + ([CROP, GO] + FRAME + [GO, COMPOSE]) * 3,
                     [CROP, GO, CROP, GO] + ([CROP, GO] + FRAME + [GO, COMPOSE]) * 3),
}
# redact, annotate and the clip calls, written from their docstrings' "per bucket" and "per frame" sentences and confirmed by this file's
# recorder on the parent of the frame-loop refactor.  A clip's pose program is captured by the call's first use of the bucket: the
# donors' landmarks in morph_clip, else the tracker ahead of the first frame.
CELLS, HULL, ROWS_T, EMA, DRAW = ['imm_redact_cells_u8', 'imm_redact_u8'], 'imm_hull_fit', 'imm_clip_rows', 'imm_clip_ema', 'imm_annotate_u8'
STATS = 'imm_colour_stats_u8'
EXPECTED['redact'] = modes(CELLS * 2, CELLS * 2, CELLS * 2)
EXPECTED['redact_hull'] = modes(([CROP] + POSE + [HULL] + CELLS) * 2, [CROP] + captured(POSE) + [HULL] + CELLS + [CROP, GO, HULL] + CELLS,
                                ([CROP, GO, HULL] + CELLS) * 2)
EXPECTED['annotate'] = {m: LANDMARKS[m] + ['imm_annotate_points', HULL, DRAW] for m in LANDMARKS}


def clip(once, frame, scores=False):
    """A clip call of three frames: `once` per call in front of the tracker, then per frame the tracker's launches and `frame`."""
    step = (['imm_landmark_scores'] if scores else []) + [STEP]
    return modes(once['eager'] + ([CROP] + POSE + step + frame) * 3, once['capture'] + ([CROP, GO] + step + frame) * 3,
                 once['replay'] + ([CROP, GO] + step + frame) * 3)


DONORS = modes([CROP] + POSE, [CROP] + captured(POSE), [CROP, GO])            # the donors' landmarks: one bucket
AHEAD = modes([], captured(POSE), [])                                         # the tracker's capture ahead of the first frame
EXPECTED['morph_clip'] = clip(DONORS, [ROWS_T] + MORPH)
EXPECTED['morph_clip_full'] = clip({m: DONORS[m] + [STATS] for m in DONORS},
                                   [ROWS_T, STATS, 'imm_colour_gain', EMA, 'imm_morph_poses', HULL, 'imm_warp_fit', 'imm_seam_fit', EMA,
                                    'imm_morph_seam_u8'])
EXPECTED['redact_clip'] = clip(AHEAD, [ROWS_T, HULL] + CELLS, scores=True)
EXPECTED['annotate_clip'] = clip(AHEAD, [HULL, DRAW])
EXPECTED['annotate_clip_track'] = modes(*[[HULL, DRAW] * 3] * 3)
# the pose photo's one row (a detector bucket of 1) in front of repose's own launches
EXPECTED['repose_pose_photos'] = modes([CROP] + POSE + EXPECTED['repose']['eager'], [CROP] + captured(POSE) + EXPECTED['repose']['capture'],
                                       [CROP, GO] + EXPECTED['repose']['replay'])


@pytest.fixture(scope='module')
def recorded():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    torch.cuda.set_device(0)
    from imm_amd import _lib
    call0 = _lib.call
    got = record(make_generator_model(K, S, 4)[1])
    from imm_amd import ops
    assert _lib.call is call0 and ops.call is call0
    return got


@pytest.mark.parametrize('mode', ['eager', 'capture', 'replay'])
def test_launch_order(recorded, mode):
    assert sorted(recorded) == sorted(EXPECTED)
    for name in EXPECTED:
        assert recorded[name][mode] == EXPECTED[name][mode], (name, mode)


if __name__ == '__main__':
    torch.cuda.set_device(0)
    got = record(make_generator_model(K, S, 4)[1])
    print('EXPECTED = {')
    for name, modes in got.items():
        print('    %r: {' % name)
        for mode, names in modes.items():
            print('        %r: %r,' % (mode, rle(names)))
        print('    },')
    print('}')
