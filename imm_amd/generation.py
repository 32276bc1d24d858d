"""Image generation with a trained model: render image y from the appearance of image x and the landmarks of y, batch norm folded.

What the reference offers is IMMModel.build(inputs, training_pl=False, build_loss=False)['future_im_pred']: a training engine per
batch size, a batch-norm pass after every encoder and renderer convolution, and image[i] paired with future_image[i] only.
ImageGenerator runs the eval-mode model as three captured stages per power-of-two bucket, each batch norm folded into the
convolution in front of it on the host in f64 (inference.fold_batch_norm), filters packed once to 16 bits, biases f32:

    appearance   image encoder, 8 x conv + bias + ReLU (inference.folded_encoder_program); conv_8 writes its 8f channels straight
                 into channels [0, 8f) of the joint buffer at He = 16, or through imm_resize_ac_fwd (align corners) at He != 16
    pose         the LandmarkDetector's own program (gen.detector): its landmarks are detect()'s, bit for bit
    render       Gaussian maps of the INPUT landmarks at 16 x 16 into channels [8f, 8f + K) of the joint buffer (render-only
                 imm_softargmax_gauss_fwd), then renderer_spec: conv + bias + ReLU blocks, imm_upsample2x_fwd after the
                 up-sampled ones, and the final conv + bias in f32 (no batch norm, no activation)

The joint buffer [n, 16, 16, Cj] is allocated zeroed; its channels [8f + K, Cj) (Cj = round_up(8f + K, 64), the padding the
deep-K kernels need) are never written.  Eval-mode batch norm is per sample, so a zero-padded bucket tail changes no result.
Nothing is written to the model: parameters, moving statistics, loss normalisers and step counters stay bit-identical.

repose() puts the generated face back where it came from: photos and face boxes in, the same photos out as u8 with every box's face
re-posed.  Per bucket the boxes are cut from the packed u8 photos (imm_resize_crop_u8 box mode), run through the appearance and render
programs, and one imm_compose_u8 launch resamples the f32 predictions to the boxes' sizes and blends them over a device copy of the
photos with a linear edge ramp (include/imm_compose.h): the f32 tiles never leave the prediction buffer.
With a template (repose(..., template=, model=)) the generator sees every face in the framing it was trained on instead of a raw box
crop: the face is aligned to the template from the original pixels (LandmarkDetector.align at So = S), encoded, rendered at a pose given
in the ALIGNED frame, and pasted back through the inverse of its alignment map (imm_unalign_maps, imm_unalign_u8; include/imm_unalign.h).
"""
import numpy as np
import torch

from . import _lib as L
from . import ops
from .engine import n_renderer_out, render_sizes, renderer_spec, trainable_spec
from .inference import (NEEDS_U8, BucketRunner, LandmarkDetector, _Launch, alloc_encoder_weights, as_image_batch, check_limits,
                        decode_u8, fold_batch_norm, folded_encoder_program, pack_folded_encoder, pack_u8, photo_boxes, photos_and_rows,
                        plan_buckets, pose_landmarks, read_variables, unalign_grid_pixels, unpack_u8)
from .keypoints import check_boxes
from .tracking import OneEuro

IMAGE_SCOPE = 'model/image_encoder'
RENDER_SCOPE = 'model/renderer'


def generator_names(cfg, image_size):
    """Variables the generator reads: (every trainable name of trainable_spec, every batch-norm block's moving statistics)."""
    params = [n for n, _shape, _wd in trainable_spec(cfg, image_size)]
    state = []
    for n in params:
        if n.endswith('/gamma'):
            sc = n[:-len('/gamma')]
            state += [sc + '/moving_mean', sc + '/moving_variance']
    return params, state


def plan_pairs(n_a, n_p, max_batch):
    """[(start, count, bucket, a_idx, p_idx)]: pairs [start, start + count) of the a-major A x P grid (pair i = (i // P, i % P))
    rendered as one program of batch `bucket`; every (a, p) is covered exactly once."""
    out = []
    for start, count, bucket in plan_buckets(n_a * n_p, max_batch):
        idx = np.arange(start, start + count)
        out.append((start, count, bucket, idx // n_p, idx % n_p))
    return out


def compose_links(rows):
    """Box rows int [n, 5] (image, y0, x0, y1, x1) of ONE imm_compose_u8 launch -> int32 [n, 2]: per row (the previous row of the
    same photo, the next one), -1 for none.  The kernel's threads find a pixel's first covering row along the first column and apply
    the later rows along the second."""
    rows = np.asarray(rows).reshape(-1, 5)
    links = np.full((len(rows), 2), -1, dtype=np.int32)
    last = {}
    for b, img in enumerate(rows[:, 0].tolist()):
        if img in last:
            links[b, 0] = last[img]
            links[last[img], 1] = b
        last[img] = b
    return links


def bucket_links(rows, buckets):
    """compose_links of every bucket (start, count, _) of rows on its own, concatenated: int32 [n, 2], one launch per bucket."""
    return np.concatenate([compose_links(rows[start:start + count]) for start, count, _b in buckets])


def box_areas(rows):
    """int64 [n]: the pixels of every box row (image, y0, x0, y1, x1)."""
    return (rows[:, 3] - rows[:, 1]).astype(np.int64) * (rows[:, 4] - rows[:, 2]).astype(np.int64)


def check_feather(feather):
    f = float(feather)
    if not 0.0 <= f <= 0.5:                          # NaN fails both comparisons
        raise ValueError('feather must lie in [0, 0.5] (the share of the box side the ramp takes), got %r' % (feather,))
    return f


def compose_inv_ramp(rows, feather):
    """f32 [n, 2]: per row the reciprocals of the edge ramp's widths feather * ih and feather * iw in pixels, and 2 where that width
    is <= 0.5 pixels (every weight is then 1: a hard paste; feather == 0 always is)."""
    f = check_feather(feather)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    ramp = f * (rows[:, 3:5] - rows[:, 1:3]).astype(np.float64)
    return np.where(ramp <= 0.5, 2.0, 1.0 / np.maximum(ramp, 0.5)).astype(np.float32)


def plan_repose(photos, poses, boxes, pose_boxes, feather, K):
    """repose()'s arguments checked on the host, before anything reaches the device: (photos as decoded u8 arrays, box rows int32
    [n, 5], poses, feather).  poses comes back as ('landmarks', f32 tensor [n or 1, K, 2]) or ('photos', decoded u8 arrays, pose_boxes)."""
    feather = check_feather(feather)
    photos, rows = photos_and_rows(photos, boxes)
    n = len(rows)
    if isinstance(poses, (list, tuple)) and len(poses) and not np.isscalar(poses[0]) and np.asarray(poses[0]).dtype == np.uint8:
        pose_photos = decode_u8(poses)
        n_p = len(pose_photos) if pose_boxes is None else len(check_boxes(pose_boxes, len(pose_photos)))
        if n_p not in (n, 1):
            raise ValueError('%d poses for %d faces: give one per face, or one for all' % (n_p, n))
        return photos, rows, ('photos', pose_photos, pose_boxes), feather
    if pose_boxes is not None:
        raise ValueError('pose_boxes need the poses as a list of u8 photos')
    lm = torch.as_tensor(poses)
    if lm.dim() != 3 or tuple(lm.shape[1:]) != (K, 2) or lm.shape[0] not in (n, 1):
        raise ValueError('poses must be landmarks [%d, %d, 2] or [1, %d, 2] (or a list of u8 pose photos), got %s' % (
            n, K, K, tuple(lm.shape)))
    return photos, rows, ('landmarks', lm.float()), feather


def check_repose_template(template, model, K, S):
    """repose(template=)'s template and model checked on the host: the similarity and affine maps are inverted, the tps map is not."""
    from . import alignment as AL
    AL.check_model(model)
    if model == 'tps':
        raise NotImplementedError('repose with a template serves the similarity and affine models; the tps map is not inverted')
    if not isinstance(template, AL.LandmarkTemplate):
        raise ValueError('template must be an alignment.LandmarkTemplate, got %r' % (type(template).__name__,))
    template.check(K, S)


def _split(names, get):
    return {n: get[n] for n in names}


class PasteSetup(object):
    """What a call that pastes faces into its photos puts on the device once, on the caller's current stream: the photos packed with
    their box rows (src, offs_d, hw_d, boxes_d: pack_u8), canvas (a copy of src to paste into; None with clone=False, for a caller
    that keeps canvases of its own), links_d (bucket_links: one launch per bucket) and ramp_d (compose_inv_ramp); area: box_areas on
    the host."""

    def __init__(self, photos, rows, buckets, feather, device, clone=True):
        self.area = box_areas(rows)
        links = bucket_links(rows, buckets)
        with torch.cuda.device(device):
            self.src, self.offs_d, self.hw_d, self.boxes_d = pack_u8(photos, device, rows)
            self.canvas = self.src.clone() if clone else None
            self.links_d = ops.to_device_pinned(links, device)
            self.ramp_d = ops.to_device_pinned(compose_inv_ramp(rows, feather), device)

    def tensors(self):
        """The device tensors, for record_stream."""
        return self.src, self.canvas, self.offs_d, self.hw_d, self.boxes_d, self.links_d, self.ramp_d

    def packed(self, part):
        """The rows `part` (a slice) as BucketRunner._stage takes them."""
        return self.src, self.offs_d, self.hw_d, self.boxes_d[part]

    def max_pixels(self, part):
        """The grid argument of a paste launch over the rows `part`: its largest box."""
        return int(min(self.area[part].max(), 2 ** 31 - 1))


class ImageGenerator(BucketRunner):
    """reconstruct(x, y) / render(x, landmarks) / transfer(appearance, poses) of a trained model (see the module docstring).
    `model` is an IMMModel whose variables exist; the generator reads them, never writes them, and refresh() re-reads them."""
    what = 'generator'

    def __init__(self, model, image_size=128, max_batch=128, use_graph=True):
        super(ImageGenerator, self).__init__(model, image_size, max_batch, use_graph)

    @classmethod
    def from_checkpoint(cls, config, path, image_size=128, max_batch=128, dtype=torch.bfloat16, device=None, use_graph=True):
        """A generator straight from a checkpoint (`.pt` file written by scripts/train.py or TensorFlow bundle prefix), without a
        training engine.  config: the `model:` block of the experiment config (config.model)."""
        cls._check(config, dtype, image_size)
        pnames, snames = generator_names(config, int(image_size))
        get = read_variables(path, pnames + snames, 'generator')
        return cls._from_variables(config, (_split(pnames, get), _split(snames, get)), image_size, max_batch, dtype, device, use_graph)

    # ------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check(cfg, dtype, image_size):
        check_limits(cfg, dtype, image_size, 'generator')
        s16 = render_sizes(cfg, int(image_size))[-1]
        if s16 != 16:
            raise NotImplementedError('renderer starts at 16x16 (min_res 16, renderer_stride 2): got %d' % s16)

    def _setup(self, cfg, dtype, device, image_size, max_batch, use_graph):
        self._check(cfg, dtype, image_size)
        if self._model is not None:
            self.detector = LandmarkDetector(self._model, image_size=image_size, max_batch=max_batch, use_graph=use_graph)
        else:
            self.detector = LandmarkDetector._from_variables(cfg, self._static, image_size, max_batch, dtype, device, use_graph)
        super(ImageGenerator, self)._setup(cfg, dtype, device, image_size, max_batch, use_graph)
        self.C8 = 8 * self.nf
        self.Cj = ops.round_up(self.C8 + self.K, 64)      # the engine's joint width: whole 64-channel K slices, zero padded
        self.n_out = n_renderer_out(cfg)
        self.rspec = renderer_spec(cfg, self.S, self.n_out)
        self.ldp = ops.round_up(self.n_out, 4)
        with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
            self.wt_im, self.bias_im = alloc_encoder_weights(self.spec, dtype, self.dev)
            self.wt_r, self.bias_r = [], []
            ci_pad = self.Cj
            for (k, _ci, co, _bn, _up) in self.rspec:
                self.wt_r.append(torch.zeros(ops.round_up(co, 128), ops.round_up(k * k * ci_pad, 32), dtype=dtype, device=self.dev))
                self.bias_r.append(torch.zeros(co, dtype=torch.float32, device=self.dev))
                ci_pad = co

    def _names(self):
        return generator_names(self.cfg, self.S)

    def refresh(self, detector=True):
        """(Re-)read the variables (the model's current ones, or the checkpoint's), fold the batch norms and re-pack the filters
        in place: captured programs stay valid.  detector=True refreshes gen.detector too."""
        variables = self._variables()
        if detector:
            self.detector.refresh()
        self._repack(*variables)

    def _pack(self, params, state):
        pack_folded_encoder(params, state, IMAGE_SCOPE, self.spec, self.wt_im, self.bias_im, self.dev)
        ci_real, ci_pad = self.C8 + self.K, self.Cj
        for i, (k, ci, co, bn, _up) in enumerate(self.rspec):
            sc = '%s/conv_%d' % (RENDER_SCOPE, i + 1)
            w, b = params[sc + '/w'].double().numpy(), params[sc + '/b'].double().numpy()
            if bn:
                w, b = fold_batch_norm(w, b, params[sc + '/gamma'], params[sc + '/beta'], state[sc + '/moving_mean'],
                                       state[sc + '/moving_variance'])
            if w.shape != (k, k, ci, co) or ci != ci_real:
                raise ValueError('%s/w: shape %s != %s' % (sc, w.shape, (k, k, ci_real, co)))
            w_dev = torch.empty(w.shape, dtype=torch.float32, device=self.dev)
            ops.upload(w_dev, torch.from_numpy(w.astype(np.float32)), sc + '/w (folded)' if bn else sc + '/w')
            rows, kpad = self.wt_r[i].shape
            ops.pack_weights(w_dev, self.wt_r[i], 0, k, k, ci_real, co, ci_pad, rows, kpad)
            ops.upload(self.bias_r[i], torch.from_numpy(b.astype(np.float32)), sc + '/b (folded)' if bn else sc + '/b')
            ci_real, ci_pad = co, co

    # ------------------------------------------------------------------------------------------------------------------------
    def _render_act_elems(self, batch):
        H, n = 16, 0
        for (_k, _ci, co, bn, up) in self.rspec:
            if bn:
                n = max(n, batch * H * H * co)
            if up:
                H *= 2
                n = max(n, batch * H * H * co)
        return n

    def _alloc(self, batch):
        self._joint = torch.zeros(batch, 16, 16, self.Cj, dtype=self.dt, device=self.dev)    # padding channels stay zero
        self._mu = torch.zeros(batch, self.K, 2, device=self.dev)
        n_r = self._render_act_elems(batch)
        self._ract = [torch.zeros(n_r, dtype=self.dt, device=self.dev) for _ in range(2)]
        self._pred = torch.zeros(batch, self.S, self.S, self.ldp, device=self.dev)

    def program(self, stage, batch):
        """The launches of one bucket of a stage: [_Launch(tag, name, family, fn)].  stage 'appearance': image rows
        -> joint channels [0, 8f); 'render': landmark rows -> Gaussian maps in the joint buffer -> renderer -> f32 prediction.
        tag: 'conv' | 'pack_image' | 'resize_ac' | 'gauss' | 'upsample'; family: the conv kernel family (imm_conv2d_variant's).
        stage 'compose': one bucket of repose(): the appearance launches, the render launches, then 'compose' (imm_compose_u8 over the
        bucket's predictions; issued by repose() with the call's photos and boxes, like the detector's 'resize')."""
        if stage == 'compose':
            return self.program('appearance', batch) + self.program('render', batch) + [_Launch('compose', 'compose_u8', 'compose', None)]
        self._ensure_capacity(batch)
        B, dt, C8, Cj = int(batch), self.dt, self.C8, self.Cj
        joint = self._joint[:B]
        if stage == 'appearance':
            direct = self.He == 16
            prog, x, H, ld = folded_encoder_program(IMAGE_SCOPE, self.spec, B, self.S, self._img[:B], self._act, self.wt_im,
                                                    self.bias_im, self._xin_for, dt, out=joint if direct else None,
                                                    ldo=Cj if direct else None)
            if not direct:       # imm_model.py:324-335: align_corners resize of the 8f-channel embedding down to 16x16
                prog.append(_Launch('resize_ac', IMAGE_SCOPE + '/resize', 'resize_ac', lambda x=x, H=H, ld=ld: ops.resize_ac_fwd(
                    x, joint, B, H, H, 16, 16, C8, ld, Cj)))
            return prog
        if stage != 'render':
            raise ValueError('stage must be appearance, render or compose, got %r' % (stage,))
        mu, mode = self._mu[:B], self.cfg.gauss_mode
        prog = [_Launch('gauss', 'gaussian_maps', 'gauss_render', lambda: ops.gauss_render_fwd(
            mu, B, self.K, self.inv_std, 16, joint[..., C8:], Cj, dt, mode))]
        x, H, ldx, ci_pad = joint, 16, Cj, Cj
        act_i = 0
        for i, (k, _ci, co, bn, up) in enumerate(self.rspec):
            name = '%s/conv_%d' % (RENDER_SCOPE, i + 1)
            if bn:
                y = self._ract[act_i][:B * H * H * co].view(B, H, H, co)
                act_i ^= 1
                d = ops.fwd_desc(B, H, H, ci_pad, ldx, co, co, k, 1, L.CONV_BIAS | L.CONV_RELU)
            else:
                y = self._pred[:B]
                d = ops.fwd_desc(B, H, H, ci_pad, ldx, co, self.ldp, k, 1, L.CONV_BIAS | L.CONV_OUT_F32)
            prog.append(_Launch('conv', name, ops.conv2d_variant(d, dt)[0],
                                (lambda d=d, x=x, y=y, i=i: ops.conv2d(d, x, self.wt_r[i], self.bias_r[i], y))))
            x, ldx, ci_pad = y, co, co
            if up:
                u = self._ract[act_i][:B * 4 * H * H * co].view(B, 2 * H, 2 * H, co)
                act_i ^= 1
                prog.append(_Launch('upsample', name + '/upsample', 'upsample', (lambda x=x, u=u, H=H, co=co: ops.upsample2x_fwd(
                    x, u, B, H, H, co, co, co))))
                x, H = u, 2 * H
        assert H == self.S
        return prog

    def _run(self, stage, batch):
        """Issue the (graph of the) program of one stage and bucket on the generator's stream."""
        self._launch((stage, batch), lambda: self.program(stage, batch))

    def _capture(self, stage, batch):
        """Make sure _run(stage, batch) finds its graph captured (BucketRunner._launch, ahead=True)."""
        self._launch((stage, batch), lambda: self.program(stage, batch), ahead=True)

    # ------------------------------------------------------------------------------------------------------------------------
    def _rows(self, images, boxes):
        """(images, u8, rows): detect()'s input forms, and with boxes (u8 photos only; keypoints.check_boxes) the photos decoded and
        the box rows int32 [n, 5] that take the images' place; rows is None without boxes."""
        if boxes is None:
            return as_image_batch(images, self.S) + (None,)
        return photo_boxes(images, boxes, self.S)

    def _encode(self, images, rows, start, count, bucket):
        """Appearance stage of images [start, start + count) into joint rows [0, count) (bucket `bucket`, tail zero images).  With
        rows (int32 [n, 5] boxes over u8 photos) the rows [start, start + count) take the images' place, cut and resized on the GPU."""
        self._stage_rows(images, rows, start, count, bucket)
        self._run('appearance', bucket)

    def _landmarks(self, landmarks, n):
        lm = torch.as_tensor(landmarks)
        if tuple(lm.shape) != (n, self.K, 2):
            raise ValueError('landmarks must be [%d, %d, 2], got %s' % (n, self.K, tuple(lm.shape)))
        return lm.to(device=self.dev, dtype=torch.float32)

    def _stage_mu(self, lm, count, bucket):
        """The render stage's input rows of one bucket: _mu[:count] = lm, the tail zero."""
        self._mu[:count].copy_(lm)
        if count < bucket:
            self._mu[count:bucket].zero_()

    def render(self, images, landmarks, boxes=None):
        """images (detect()'s forms, N of them) rendered at landmarks f32 [N, K, 2] ((y, x) in [-1, 1]): f32 [N, S, S, 3],
        unclipped, in the 0..255 scale of future_im_pred.  boxes (as keypoints() takes them, u8 photos only): the N rows are the
        boxes, cut from their photos with zero padding and resized to S x S on the GPU."""
        images, _u8, rows = self._rows(images, boxes)
        N = len(images) if rows is None else len(rows)
        lm = self._landmarks(landmarks, N)
        out = torch.empty(N, self.S, self.S, 3, device=self.dev)
        with self._forked():
            for start, count, bucket in plan_buckets(N, self.max_batch):
                self._encode(images, rows, start, count, bucket)
                self._stage_mu(lm[start:start + count], count, bucket)
                self._run('render', bucket)
                out[start:start + count].copy_(self._pred[:count, ..., :3])
        return out

    def reconstruct(self, images, future_images, boxes=None, pose_boxes=None):
        """future_images rendered from the appearance of images (pair i = (images[i], future_images[i])): f32 [N, S, S, 3], the
        eval path's future_im_pred.  boxes / pose_boxes (u8 photos only): the rows of either side are its boxes (row i of one pairs
        with row i of the other)."""
        images, _, rows = self._rows(images, boxes)
        future_images, _, prows = self._rows(future_images, pose_boxes)
        n, n_f = (len(images) if rows is None else len(rows)), (len(future_images) if prows is None else len(prows))
        if n != n_f:
            raise ValueError('images and future_images differ in number: %d != %d' % (n, n_f))
        mu = self.detector.detect(future_images) if prows is None else self.detector.landmarks(future_images, pose_boxes)
        return self.render(images, mu, boxes=boxes)

    def transfer(self, appearance, poses, return_landmarks=False, boxes=None, pose_boxes=None):
        """Every appearance image rendered at every pose image's landmarks: f32 [A, P, S, S, 3], [a, p] = reconstruct(appearance[a],
        poses[p]).  Each image is encoded once (the appearance stage per A bucket, the detector per P bucket); the A x P pairs are
        rendered in buckets, their joint rows gathered from the stored features.  return_landmarks=True: (images, the poses'
        landmarks f32 [P, K, 2] it rendered at).  boxes / pose_boxes (u8 photos only): the A appearance rows / the P pose rows are
        the boxes of those photos."""
        appearance, _u8, rows = self._rows(appearance, boxes)
        n_a = len(appearance) if rows is None else len(rows)
        if pose_boxes is None:
            mu_p = self.detector.detect(poses)
        else:
            if not isinstance(poses, (list, tuple)):
                raise ValueError(NEEDS_U8)
            mu_p = self.detector.landmarks(poses, pose_boxes)
        n_p = mu_p.shape[0]
        out = torch.empty(n_a * n_p, self.S, self.S, 3, device=self.dev)
        with self._forked():
            feats = torch.empty(n_a, 16, 16, self.C8, dtype=self.dt, device=self.dev)
            for start, count, bucket in plan_buckets(n_a, self.max_batch):
                self._encode(appearance, rows, start, count, bucket)
                feats[start:start + count].copy_(self._joint[:count, ..., :self.C8])
            for start, count, bucket, a_idx, p_idx in plan_pairs(n_a, n_p, self.max_batch):
                self._ensure_capacity(bucket)
                a_idx = torch.from_numpy(a_idx).to(self.dev)
                p_idx = torch.from_numpy(p_idx).to(self.dev)
                self._joint[:count, ..., :self.C8].copy_(feats.index_select(0, a_idx))
                if count < bucket:
                    self._joint[count:bucket, ..., :self.C8].zero_()
                self._stage_mu(mu_p.index_select(0, p_idx), count, bucket)
                self._run('render', bucket)
                out[start:start + count].copy_(self._pred[:count, ..., :3])
        out = out.view(n_a, n_p, self.S, self.S, 3)
        return (out, mu_p) if return_landmarks else out

    def repose(self, photos, poses, boxes=None, pose_boxes=None, feather=0.125, return_faces=False, template=None, model='similarity'):
        """The photos with every box's face re-posed: a list of u8 device tensors [h_i, w_i, 3], one per photo, views of one packed
        buffer.  photos: a list of u8 arrays of any sizes (decode_u8's forms).  boxes: as keypoints() takes them, n rows; by default
        one whole-photo box per photo.  poses: landmarks f32 [n, K, 2] (or [1, K, 2] for all rows), or a list of u8 pose photos whose
        landmarks are detector.landmarks(poses, pose_boxes), n rows or 1.  feather in [0, 0.5]: the share of each box side over which
        the paste fades into the photo (0: a hard paste).  return_faces=True: (photos, faces f32 [n, S, S, 3], landmarks f32 [n, K, 2]).
        Every row's crop is cut from the ORIGINAL pixels and the faces are composited into a device copy, in row order (a later box
        blends over an earlier paste, imm_compose_u8's rule): an overlapping later box never sees an earlier paste in its crop.  A
        face is resampled bilinearly, without a pre-filter: a box much smaller than S x S point-samples its face.
        template (an alignment.LandmarkTemplate of this model's K and S) with model 'similarity' | 'affine': every face is first
        aligned to the template from the original u8 pixels (detector.align at So = S), so the generator sees the framing it was
        trained on; it is encoded, rendered at its pose and pasted back through the inverse of its alignment map (imm_unalign_u8),
        feather being a share of the ALIGNED frame's side.  The poses are then landmarks in the aligned frame; pose photos give
        detector.detect(detector.align(pose_photos, template, pose_boxes, model)).  'tps' raises NotImplementedError (the tps map is
        not inverted).  return_faces=True returns the aligned-frame renders and those landmarks."""
        if template is not None:
            return self._repose_aligned(photos, poses, boxes, pose_boxes, feather, return_faces, template, model)
        S = self.S
        photos, rows, pose, feather = plan_repose(photos, poses, boxes, pose_boxes, feather, self.K)
        n = len(rows)
        lm = pose_landmarks(self.detector, pose, n)
        buckets = plan_buckets(n, self.max_batch)
        ps = PasteSetup(photos, rows, buckets, feather, self.dev)                   # all photos, once per call
        faces = torch.empty(n, S, S, 3, device=self.dev) if return_faces else None
        with self._forked(*ps.tensors()):
            for start, count, bucket in buckets:
                part = slice(start, start + count)
                self._stage(count, bucket, packed=ps.packed(part))
                self._stage_mu(lm[part], count, bucket)
                self._run('appearance', bucket)
                self._run('render', bucket)
                ops.compose_u8(ps.canvas, ps.offs_d, ps.hw_d, ps.boxes_d[part], ps.links_d[part], ps.ramp_d[part], self._pred[:count],
                               ps.max_pixels(part))
                if return_faces:
                    faces[part].copy_(self._pred[:count, ..., :3])
        out = unpack_u8(ps.canvas, photos)
        return (out, faces, lm.contiguous()) if return_faces else out

    def reenact(self, photos, frames, driver_box, boxes=None, motion='relative', rigid=True, gain=1.0, smooth=True, feather=0.125,
                paste=True, box_smooth=0.5, one_euro=OneEuro(), fps=25.0, chunk_frames=32, return_faces=False, template=None, model=None):
        """A driving clip animates the faces of still photos: a reenact.Reenactment (landmarks f32 [T, n, K, 2] the poses rendered,
        flags int32 [T, n] / held, faces f32 [T, n, S, S, 3] with return_faces=True, frames[t][i] photo i at frame t as u8 [h_i, w_i, 3]
        with paste=True, track the driver's tracking.Track) on the generator's device.
        photos / boxes: as repose() takes them, n rows, n <= max_batch.  frames / driver_box: a clip, a list of T u8 HWC arrays, and the
        ONE driving face (y0, x0, y1, x1) of its first frame, as detector.track takes them (box_smooth, one_euro, fps, chunk_frames
        likewise).  motion 'relative': the driver's motion since its first frame is added to each face's own landmarks; 'absolute': the
        driver's shape itself is laid over each face.  rigid=False: the driver's head motion (turn, size, shift) is divided out first, so
        only its expression moves the faces.  gain in [0, 4] scales the motion (0: the faces' own poses).  smooth=False reads the
        tracker's raw points instead of its One-Euro filtered ones.  feather: as in repose().
        The photos are uploaded, cut and encoded once; per frame the tracker's launches, imm_retarget (include/imm_retarget.h states
        the rule), the captured render program and one imm_compose_u8 launch are queued, and nothing returns to the host between the
        clip's first and last launch (imm_amd/reenact.py).  A face whose rule has no usable answer on a frame, and every face on a frame
        that lost the driver, keeps its pose of the frame before (flags bit 0).  template= (re-enactment in the aligned frame), model=
        (tps, affine) and several drivers are not implemented and raise."""
        from . import reenact as RE
        plan = RE.plan_reenact(photos, frames, driver_box, boxes, self.max_batch, motion, rigid, gain, smooth, feather, paste, box_smooth,
                               one_euro, fps, chunk_frames, template, model)
        return RE.run(self, plan, return_faces)

    def _repose_aligned(self, photos, poses, boxes, pose_boxes, feather, return_faces, template, model):
        """repose() with a template: align -> encode -> render -> paste through the inverse map.  The photos are packed once: the
        detector's align() reads that buffer, and since every face is aligned before the first paste the same buffer is pasted into."""
        from . import alignment as AL
        S, det = self.S, self.detector
        check_repose_template(template, model, self.K, S)
        photos, rows, pose, feather = plan_repose(photos, poses, boxes, pose_boxes, feather, self.K)
        n = len(rows)
        lm = pose_landmarks(det, pose, n, lambda p, b: det.detect(det.align(p, template, b, model)))
        buckets = plan_buckets(n, self.max_batch)
        links = bucket_links(rows, buckets)
        with torch.cuda.device(self.dev):
            canvas, offs_d, hw_d, boxes_d = pack_u8(photos, self.dev, rows)         # all photos, once per call
            links_d = ops.to_device_pinned(links, self.dev)
            aligned, al = det.align(photos, template, rows, model, return_transform=True, _packed=(canvas, offs_d, hw_d, boxes_d))
            fwd = torch.empty(n, 6, device=self.dev)
            bbox = torch.empty(n, 4, dtype=torch.int32, device=self.dev)
            ops.unalign_maps(al.coef, al.geom, boxes_d, hw_d, S, S, fwd, bbox)      # the coefficients never leave the device
            faces = torch.empty(n, S, S, 3, device=self.dev) if return_faces else None
        inv_ramp = AL.unalign_inv_ramp(feather, S)
        with self._forked(canvas, offs_d, hw_d, boxes_d, links_d, aligned, fwd, bbox):
            for start, count, bucket in buckets:
                part = slice(start, start + count)
                self._stage(count, bucket, aligned[part])
                self._stage_mu(lm[part], count, bucket)
                self._run('appearance', bucket)
                self._run('render', bucket)
                ops.unalign_u8(canvas, offs_d, hw_d, boxes_d[part], links_d[part], fwd[part], bbox[part], inv_ramp, self._pred[:count],
                               unalign_grid_pixels(photos, rows[part]))
                if return_faces:
                    faces[part].copy_(self._pred[:count, ..., :3])
        out = unpack_u8(canvas, photos)
        return (out, faces, lm.contiguous()) if return_faces else out
