"""Landmark detection with a trained model: the pose encoder alone, batch norm folded into the convolutions.

What the reference offers for detection is IMMModel.build(training_pl=False, build_loss=False): the whole model in eval mode
(both encoders and the renderer) to read off `gauss_yx`, which depends on the pose encoder only.  On this build that path is a
training engine per batch size (flat gradients, optimizer slots, VGG weights, every training activation) and every pose-encoder
block is a 16-bit conv output followed by a batch-norm pass over it.

In eval mode the batch norm of a block is a per-channel affine map with the moving statistics, so it folds into the convolution
in front of it (host, f64, once per construction or refresh()):

    s = gamma / sqrt(moving_variance + BN_EPS),   W' = W * s,   b' = (b - moving_mean) * s + beta
    relu(BN_eval(conv(x, W) + b)) == relu(conv(x, W') + b')

W' is packed to 16 bits once (imm_pack_weights: one rounding per weight, like the training engine's W), b' stays f32.  A batch
of images is then 10 launches, captured into a HIP graph per power-of-two batch bucket:

    [imm_resize_crop_u8]          u8 images of any size -> f32 S x S (TF1 bilinear, align_corners; list input only, issued
                                  ahead of the graph because the packed pixel buffer changes from call to call)
    conv_1 7x7, 3 -> f            imm_conv_first with BIAS | RELU (straight from the f32 image; tap-unrolled 7x1 form where
                                  imm_conv_first_supported says no)
    conv_2 .. conv_8              imm_conv2d with BIAS | RELU (the kernel family imm_conv2d_variant names)
    pose head                     imm_pose_head_fwd: 1x1 conv 8f -> K, soft-argmax -> heat maps and mu

No statistics, no batch-norm launches, nothing written back to the model: parameters, moving statistics, loss normalisers,
step counters stay bit-identical.  Eval-mode batch norm is per sample, so the zero-padded tail of a bucket cannot change a result.
"""
import contextlib

import numpy as np
import torch

from . import _lib as L
from . import ops
from .engine import BN_EPS, encoder_spec
from .keypoints import box_geometry, check_boxes
from .tracking import OneEuro

POSE_SCOPE = 'model/pose_encoder'
MAX_LANDMARKS = 64            # the soft-argmax / pose-head kernels' limit


def fold_batch_norm(w, b, gamma, beta, moving_mean, moving_variance, eps=BN_EPS):
    """(W', b') in f64 with conv(x, W') + b' == BN_eval(conv(x, W) + b); w is HWIO [kh, kw, ci, co], the rest [co]."""
    w = np.asarray(w, dtype=np.float64)
    b, gamma, beta, mm, mv = (np.asarray(v, dtype=np.float64) for v in (b, gamma, beta, moving_mean, moving_variance))
    s = gamma / np.sqrt(mv + eps)
    return w * s, (b - mm) * s + beta


def bucket_sizes(max_batch):
    """The batch sizes a detector captures programs for: powers of two below max_batch, and max_batch itself."""
    if max_batch < 1:
        raise ValueError('max_batch must be >= 1, got %r' % (max_batch,))
    return [1 << i for i in range(max_batch.bit_length()) if (1 << i) < max_batch] + [int(max_batch)]


def plan_buckets(n, max_batch):
    """[(start, count, bucket)]: images [start, start + count) run as one program of batch `bucket` (count <= bucket <=
    max_batch; the bucket's last bucket - count rows are zero padding).  Every image is covered exactly once."""
    sizes = bucket_sizes(int(max_batch))
    out, start = [], 0
    while start < n:
        count = min(int(max_batch), n - start)
        out.append((start, count, next(s for s in sizes if s >= count)))
        start += count
    return out


def encoder_names(scope, n_filters):
    """(parameter names, batch-norm state names) of one encoder's eight conv + BN blocks, engine / checkpoint naming."""
    params, state = [], []
    for i in range(len(encoder_spec(n_filters))):
        sc = '%s/encoder/conv_%d' % (scope, i + 1)
        params += [sc + '/w', sc + '/b', sc + '/gamma', sc + '/beta']
        state += [sc + '/moving_mean', sc + '/moving_variance']
    return params, state


def pose_encoder_names(n_filters):
    """Variables the detector reads: (parameter names, batch-norm state names), engine / checkpoint naming."""
    params, state = encoder_names(POSE_SCOPE, n_filters)
    params += [POSE_SCOPE + '/conv_1/w', POSE_SCOPE + '/conv_1/b']
    return params, state


def read_variables(path, names, what='model'):
    """The named variables of a checkpoint as host f32 tensors {name: tensor}: a `.pt` file written by scripts/train.py
    ({'params', 'state'}) or the prefix of a TensorFlow bundle (`<prefix>.index` next to it; the reference's released checkpoints)."""
    import os
    names = list(names)
    if os.path.isfile(path + '.index'):
        from .utils.tf_checkpoint import read_bundle, tf_variable_name
        want = {tf_variable_name(n): n for n in names}
        data = read_bundle(path, names=set(want))
        missing = [t for t in want if t not in data]
        if missing:
            raise KeyError('%s lacks %d %s variables (e.g. %s)' % (path, len(missing), what, missing[0]))
        get = {n: torch.from_numpy(np.asarray(data[t], dtype=np.float32)) for t, n in want.items()}
    elif os.path.isfile(path):
        ck = torch.load(path, map_location='cpu')
        src = dict(ck['params'])
        src.update(ck.get('state') or {})
        missing = [n for n in names if n not in src]
        if missing:
            raise KeyError('%s lacks %d %s variables (e.g. %s)' % (path, len(missing), what, missing[0]))
        get = {n: torch.as_tensor(src[n], dtype=torch.float32) for n in names}
    else:
        raise FileNotFoundError('checkpoint %s not found (neither a file nor a TensorFlow bundle prefix)' % path)
    return {n: get[n] for n in names}


def read_checkpoint(path, n_filters):
    """Pose-encoder variables of a checkpoint as host f32 tensors (params, state): see read_variables."""
    pnames, snames = pose_encoder_names(n_filters)
    get = read_variables(path, pnames + snames, 'pose-encoder')
    return {n: get[n] for n in pnames}, {n: get[n] for n in snames}


def alloc_encoder_weights(spec, dtype, device):
    """Packed-filter images and folded-bias vectors of a folded encoder (zeros; filled by pack_folded_encoder)."""
    wt, bias = [], []
    for i, (k, ci, co, _st) in enumerate(spec):
        kpad = ops.round_up(7 * 32, 32) if i == 0 else ops.round_up(k * k * ci, 32)
        wt.append(torch.zeros(ops.round_up(co, 128), kpad, dtype=dtype, device=device))
        bias.append(torch.zeros(co, dtype=torch.float32, device=device))
    return wt, bias


def pack_folded_encoder(params, state, scope, spec, wt, bias, device):
    """Fold every block's eval-mode batch norm into its convolution (host, f64) and pack the filters in place (current stream)."""
    for i, (k, ci, co, _st) in enumerate(spec):
        sc = '%s/encoder/conv_%d' % (scope, i + 1)
        g = lambda n: params[sc + '/' + n].double().numpy()
        wf, bf = fold_batch_norm(g('w'), g('b'), g('gamma'), g('beta'), state[sc + '/moving_mean'].double().numpy(),
                                 state[sc + '/moving_variance'].double().numpy())
        if wf.shape != (k, k, ci, co):
            raise ValueError('%s/w: shape %s != %s' % (sc, wf.shape, (k, k, ci, co)))
        w_dev = torch.empty(wf.shape, dtype=torch.float32, device=device)
        ops.upload(w_dev, torch.from_numpy(wf.astype(np.float32)), sc + '/w (folded)')
        rows, kpad = wt[i].shape
        if i == 0:      # HWIO [7, 7, 3, co] is [7, 1, 21, co]: the tap-unrolled 7x1 filter image both conv_1 forms read
            ops.pack_weights(w_dev, wt[i], 0, k, 1, 3 * k, co, 32, rows, kpad)
        else:
            ops.pack_weights(w_dev, wt[i], 0, k, k, ci, co, ci, rows, kpad)
        ops.upload(bias[i], torch.from_numpy(bf.astype(np.float32)), sc + '/b (folded)')


def encoder_act_elems(spec, S, batch):
    """Elements of the larger ping-pong activation buffer a folded encoder of this batch needs."""
    out, f = 0, 1
    for (_k, _ci, co, st) in spec:
        f *= st
        out = max(out, batch * (S // f) ** 2 * co)
    return out


def folded_encoder_program(scope, spec, B, S, img, act, wt, bias, xin_for, dt, out=None, ldo=None):
    """The launches of a folded encoder over B images f32 [B, S, S, 3] (`img`): conv_1 straight from the f32 image (imm_conv_first;
    the tap-unrolled 7x1 form where it says no), conv_2 .. conv_8 by imm_conv2d, every one with BIAS | RELU; outputs ping-pong
    between the two flat buffers `act`.  out / ldo: where conv_8 writes (pixel stride ldo), e.g. the renderer's joint buffer.
    Returns (launches, last output, its side, its pixel stride)."""
    prog = []
    x, H, ld = None, S, 3
    for i, (k, ci_, co, st) in enumerate(spec):
        name = '%s/encoder/conv_%d' % (scope, i + 1)
        Ho = -(-H // st)
        if out is not None and i == len(spec) - 1:
            y, ldy = out, ldo
        else:
            y, ldy = act[i % 2][:B * Ho * Ho * co].view(B, Ho, Ho, co), co
        if i == 0:
            if ops.conv_first_supported(B, S, co, ldy):
                prog.append(_Launch('conv', name, 'first', (lambda y=y, i=i, co=co, ldy=ldy: ops.conv_first(
                    img, wt[i], bias[i], y, ldy, None, B, S, co, L.CONV_BIAS | L.CONV_RELU))))
            else:
                xin = xin_for(B)
                prog.append(_Launch('pack_image', name + '/pack', 'pack_image',
                                    lambda xin=xin: ops.pack_image_taps(img, xin, B, S, S, 7, 3, 32)))
                d = ops.fwd_desc(B, S, S, 32, 32, co, ldy, 7, 1, L.CONV_BIAS | L.CONV_RELU, kw=1)
                prog.append(_Launch('conv', name, ops.conv2d_variant(d, dt)[0],
                                    (lambda d=d, xin=xin, y=y, i=i: ops.conv2d(d, xin, wt[i], bias[i], y))))
        else:
            d = ops.fwd_desc(B, H, H, ci_, ld, co, ldy, k, st, L.CONV_BIAS | L.CONV_RELU)
            prog.append(_Launch('conv', name, ops.conv2d_variant(d, dt)[0],
                                (lambda d=d, x=x, y=y, i=i: ops.conv2d(d, x, wt[i], bias[i], y))))
        x, H, ld = y, Ho, ldy
    return prog, x, H, ld


def check_limits(cfg, dtype, image_size, what='detector'):
    """The folded inference paths' limits (16-bit storage, S a multiple of 16 and >= 64, 1..64 landmarks): (S, K, n_filters)."""
    if dtype == torch.float32:
        raise NotImplementedError('the landmark %s runs the 16-bit kernels (bf16 / f16); the f32 witness engine is a '
                                  'test instrument without one' % what)
    ops.dtype_enum(dtype)
    S = int(image_size)
    if S % 16 or S < 64:
        raise ValueError('image side must be a multiple of 16 and >= 64')
    K, nf = int(cfg.n_maps), int(cfg.n_filters)
    if not 1 <= K <= MAX_LANDMARKS:
        raise NotImplementedError('the %s serves 1..%d landmarks (the soft-argmax limit), got %d' % (what, MAX_LANDMARKS, K))
    ops.gauss_mode_enum(cfg.gauss_mode)
    return S, K, nf


def as_image_batch(images, S):
    """detect()'s input forms: (NHWC float tensor [N, S, S, 3] in [0, 255] (host or device), False) or (list of u8 arrays, True)."""
    u8 = isinstance(images, (list, tuple))
    if not u8:
        images = torch.as_tensor(images)
        if images.dim() != 4 or tuple(images.shape[1:]) != (S, S, 3):
            raise ValueError('images must be [N, %d, %d, 3], got %s' % (S, S, tuple(images.shape)))
        if images.is_cuda and images.dtype != torch.float32:
            images = images.float()
    return images, u8


def decode_u8(images):
    """detect()'s u8 input arrays as contiguous HxWx3 u8 arrays (grey images repeated to three channels)."""
    decoded = []
    for a in images:
        a = np.asarray(a)
        if a.dtype != np.uint8:
            raise TypeError('image arrays must be uint8 HWC, got %s' % a.dtype)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3 or a.shape[2] not in (1, 3):
            raise ValueError('image arrays must be HxW, HxWx1 or HxWx3, got shape %s' % (a.shape,))
        if a.shape[2] == 1:
            a = np.repeat(a, 3, axis=2)
        decoded.append(np.ascontiguousarray(a))
    return decoded


def packed_offsets(decoded):
    """Where pack_u8 puts each of the decoded images (16-byte aligned starts): (offsets i64 [count], the bytes they take)."""
    offs = np.zeros(len(decoded), dtype=np.int64)
    total = 0
    for i, a in enumerate(decoded):
        offs[i] = total
        total += (a.size + 15) & ~15
    return offs, total


def unpack_u8(packed, decoded):
    """The images of a buffer laid out as pack_u8(decoded) lays it out: a list of views [h_i, w_i, 3], one per image."""
    return [packed[o:o + a.size].view(a.shape) for o, a in zip(packed_offsets(decoded)[0].tolist(), decoded)]


def pack_u8(images, device, boxes=None):
    """Pack u8 HWC images back to back (16-byte aligned starts, like the data loader) into one device buffer: (src u8, offsets i64
    [count], hw i32 [count, 2], boxes i32 [n, 5] or None), what imm_resize_crop_u8 and imm_align_warp_u8 read."""
    decoded = decode_u8(images)
    count = len(decoded)
    offs, total = packed_offsets(decoded)
    packed = np.zeros(max(total, 16), dtype=np.uint8)
    for a, o in zip(decoded, offs):
        packed[o:o + a.size] = a.reshape(-1)
    hw = np.array([a.shape[:2] for a in decoded], dtype=np.int32)
    src = ops.to_device_pinned(packed, device)
    offs_d = ops.to_device_pinned(offs, device)
    hw_d = ops.to_device_pinned(hw, device)
    boxes_d = None if boxes is None else ops.to_device_pinned(np.ascontiguousarray(boxes, dtype=np.int32), device)
    return src, offs_d, hw_d, boxes_d


def stage_u8(images, dst, S, device, boxes=None):
    """Pack u8 HWC images (pack_u8) and resize them on the GPU (TF1 bilinear, align_corners) into dst f32 [len(images), S, S, 3]
    (current stream).  boxes: int32 [n, 5] rows (image, y0, x0, y1, x1) checked by keypoints.check_boxes: dst row b is then box b cut
    from images[boxes[b][0]] (zero-padded) and resized, dst [n, S, S, 3].  Returns the packed device tensors."""
    src, offs_d, hw_d, boxes_d = pack_u8(images, device, boxes)
    ops.resize_crop_u8(src, offs_d, hw_d, 3, (S, S), (0, 0), (S, S), dst, boxes=boxes_d)
    return src, offs_d, hw_d, boxes_d


UNALIGN_MAX_ROWS = 65535      # rows of one imm_unalign_u8 launch (its grid's y dimension)


def plan_unalign(photos, aligned_shape, alignment, feather):
    """unalign()'s arguments checked on the host, before anything reaches the device: (photos as decoded u8 arrays, the alignment's
    box rows int32 [n, 5], n, So, feather)."""
    from .generation import check_feather
    if alignment.model == 'tps':
        raise NotImplementedError('unalign serves the similarity and affine models; the tps map is not inverted')
    feather = check_feather(feather)
    rows = getattr(alignment, 'rows', None)
    if rows is None:
        raise ValueError('the alignment holds no box rows: unalign needs what align(u8 photos, ..., return_transform=True) returns')
    if not isinstance(photos, (list, tuple)):
        raise ValueError('unalign needs the photos as the list of u8 arrays align() was given')
    photos = decode_u8(photos)
    n, So = len(rows), int(alignment.out_size)
    shape = tuple(int(v) for v in aligned_shape)
    if len(shape) != 4 or shape[1:3] != (So, So) or shape[3] < 3:
        raise ValueError('aligned must be [n, %d, %d, >= 3] (the alignment\'s out_size), got %s' % (So, So, shape))
    if shape[0] != n or len(alignment.coef) != n or len(alignment.geom) != n:
        raise ValueError('%d aligned faces, %d coefficient rows and %d geometry rows for the alignment\'s %d box rows' % (
            shape[0], len(alignment.coef), len(alignment.geom), n))
    if n == 0:
        raise ValueError('the alignment holds no rows')
    if tuple(np.shape(alignment.coef)[1:]) != (3, 2):
        raise ValueError('coef must be [n, 3, 2], got %s' % (tuple(np.shape(alignment.coef)),))
    if rows[:, 0].min() < 0 or rows[:, 0].max() >= len(photos):
        raise ValueError('the alignment\'s rows name photos 0..%d, %d photos were given' % (int(rows[:, 0].max()), len(photos)))
    return photos, rows, n, So, feather


def unalign_grid_pixels(photos, rows):
    """The max_pixels of an imm_unalign_u8 launch over these box rows, from what the host knows: twice the largest box (an aligned face
    covers about its box; its bounding box, once rotated, up to twice that), at most the largest photo the rows name.  It sizes the
    grid only: a larger bounding box is still pasted whole."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    box = int(((rows[:, 3] - rows[:, 1]) * (rows[:, 4] - rows[:, 2])).max())
    photo = max(int(photos[i].shape[0]) * int(photos[i].shape[1]) for i in set(rows[:, 0].tolist()))
    return int(max(1, min(2 * max(box, 1), photo, 2 ** 31 - 1)))


NEEDS_U8 = 'boxes need the images as a list of u8 arrays (a tensor batch is already S x S)'


def local_rows(part):
    """The box rows int32 [n, 5] of one bucket renumbered into the photos they use: (used, local) with `used` the sorted indices of
    those photos (each packed once) and `local` the rows with column 0 indexing into `used`."""
    used, idx = np.unique(part[:, 0], return_inverse=True)
    return used, np.concatenate([idx.reshape(-1, 1).astype(np.int32), part[:, 1:]], axis=1)


def photo_boxes(images, boxes, S):
    """keypoints()'s input forms resolved: (images, u8, rows).  A list of u8 photos comes back decoded, with its box rows int32 [n, 5]
    (keypoints.check_boxes; one whole-photo box per photo without boxes).  A tensor batch [N, S, S, 3] takes no boxes and has no rows."""
    images, u8 = as_image_batch(images, S)
    if not u8:
        if boxes is not None:
            raise ValueError(NEEDS_U8)
        return images, False, None
    images = decode_u8(images)
    return images, True, check_boxes([(0, 0, a.shape[0], a.shape[1]) for a in images] if boxes is None else boxes, len(images))


def photos_and_rows(photos, boxes, needs=NEEDS_U8, empty=None, not_u8=TypeError, limit=None):
    """What every plan_* does with a list of u8 photos and optional boxes: (photos decoded (decode_u8), box rows int32 [n, 5]
    (keypoints.check_boxes; one whole-photo box per photo without boxes)).  The refusals are worded by the caller: needs, the ValueError
    for photos that are no list; empty, the ValueError for an empty list (None: the list goes on to check_boxes); not_u8, the type
    decode_u8's TypeError is raised as; limit = (rows, text with one %d for the count): the ValueError for more rows than that."""
    if not isinstance(photos, (list, tuple)):
        raise ValueError(needs)
    if empty is not None and not len(photos):
        raise ValueError(empty)
    try:
        photos = decode_u8(photos)
    except TypeError as e:
        raise not_u8(str(e))
    rows = check_boxes([(0, 0, a.shape[0], a.shape[1]) for a in photos] if boxes is None else boxes, len(photos))
    if limit is not None and len(rows) > limit[0]:
        raise ValueError(limit[1] % len(rows))
    return photos, rows


def check_landmarks(landmarks, counts, K, name='landmarks'):
    """landmarks given by a caller: an f32 tensor [n, K, 2] with n one of counts, where it lies; values are not looked at."""
    t = torch.as_tensor(landmarks)
    if t.dim() != 3 or tuple(t.shape[1:]) != (int(K), 2) or t.shape[0] not in counts:
        raise ValueError('%s must be [%s, %d, 2], got %s' % (name, ' or '.join(str(c) for c in counts), int(K), tuple(t.shape)))
    return t.float()


def photo_rows(images, boxes, S):
    """photo_boxes and the rows' geometry f32 [n, 4] (keypoints.box_geometry; (0, 0, 1, 1) per image of a tensor batch):
    (images, u8, rows, geom)."""
    images, u8, rows = photo_boxes(images, boxes, S)
    geom = box_geometry(rows, S) if u8 else np.tile(np.array([0, 0, 1, 1], np.float32), (len(images), 1))
    return images, u8, rows, geom


def pose_landmarks(detector, pose, n, from_photos=None):
    """A pose source as generation.plan_repose returns it -> landmarks f32 [n, K, 2] on the detector's device: ('landmarks', tensor
    [n or 1, K, 2]) is moved there, ('photos', u8 photos, boxes) goes through from_photos(photos, boxes) (default: detector.landmarks);
    one row is expanded (a view) to n."""
    if pose[0] == 'photos':
        lm = (from_photos or detector.landmarks)(pose[1], pose[2])
    else:
        lm = pose[1].to(device=detector.dev, dtype=torch.float32)
    return lm.expand(n, detector.K, 2) if lm.shape[0] != n else lm


class _Held(list):
    """The device tensors a call allocates on the caller's stream and uses on the object's: the record list of BucketRunner._forked
    and of tracking.run_frames, complete because every such tensor is made through it.  keep(tensors...) takes tensors made elsewhere (pack_u8's, a PasteSetup's; None
    is skipped), up(array) uploads one (ops.to_device_pinned), empty(*shape) and zeros(*shape) allocate one; each returns what it holds."""

    def __init__(self, device):
        super(_Held, self).__init__()
        self.device = device

    def keep(self, *tensors):
        self.extend(t for t in tensors if t is not None)
        return tensors[0] if len(tensors) == 1 else tensors

    def up(self, array):
        return self.keep(ops.to_device_pinned(array, self.device))

    def empty(self, *shape, **kw):
        return self.keep(torch.empty(*shape, device=self.device, **kw))

    def zeros(self, *shape, **kw):
        return self.keep(torch.zeros(*shape, device=self.device, **kw))


class _Plan(object):
    """The checked arguments of a call, by name: a plan_* function's result.  A subclass names its FIELDS; a field that is missing
    or misspelt fails here, where the plan is made."""
    FIELDS = ()

    def __init__(self, **fields):
        assert set(fields) == set(self.FIELDS), sorted(set(fields) ^ set(self.FIELDS))
        self.__dict__.update(fields)


class _Launch(object):
    __slots__ = ('tag', 'name', 'family', 'fn')

    def __init__(self, tag, name, family, fn):
        self.tag, self.name, self.family, self.fn = tag, name, family, fn


class BucketRunner(object):
    """What LandmarkDetector and ImageGenerator share: a folded encoder run in power-of-two batch buckets on the object's own stream.
    It owns the construction state (cfg, dt, dev, S, K, nf, max_batch, use_graph, He, inv_std, spec, stream, _stager), the buffers of
    one bucket sized for the largest bucket run so far (_img, _xin, _act; the subclass's in _alloc), the graph cache (_graphs, dropped
    whenever the buffers are reallocated), the staging of a bucket's input rows (_stage) and the fork to the object's stream and back
    (_forked).  A subclass says what it reads (_names), how it packs it (_pack), what else a bucket needs (_alloc) and its launches
    (program, _run) and the word for itself in error messages (what)."""

    def __init__(self, model, image_size, max_batch, use_graph):
        eng = getattr(model, '_master', None) or getattr(model, 'engine', None)
        if eng is None:
            raise RuntimeError('the model has no variables yet: build, train or restore it first '
                               '(or use %s.from_checkpoint)' % type(self).__name__)
        self._model, self._static = model, None
        self._setup(model._config, model.dtype, eng.dev, image_size, max_batch, use_graph)
        self._repack(*self._variables())

    @classmethod
    def _from_variables(cls, config, static, image_size, max_batch, dtype, device, use_graph):
        """An object over host variables (params, state) that it keeps for refresh()."""
        obj = cls.__new__(cls)
        obj._model, obj._static = None, static
        if device is None:
            device = 'cuda:%d' % torch.cuda.current_device()
        obj._setup(config, dtype, torch.device(device), image_size, max_batch, use_graph)
        obj._repack(*obj._variables())
        return obj

    def _setup(self, cfg, dtype, device, image_size, max_batch, use_graph):
        S, K, nf = check_limits(cfg, dtype, image_size, self.what)
        L.load()
        self.cfg, self.dt, self.dev, self.S, self.K, self.nf = cfg, dtype, torch.device(device), S, K, nf
        self.max_batch = int(max_batch)
        bucket_sizes(self.max_batch)
        self.use_graph = bool(use_graph)
        self.He = S // 8
        self.inv_std = 1.0 / float(cfg.gauss_std)
        self.spec = encoder_spec(nf)
        self.stream = torch.cuda.Stream(device=self.dev)
        self._stager = ops.PinnedStager()
        self._cap = 0
        self._graphs = {}

    def _variables(self):
        """(params, state) of _names() as host tensors: the stored checkpoint's, or the live engine's current ones."""
        if self._static is not None:
            return self._static
        eng = getattr(self._model, '_master', None) or self._model.engine
        pnames, snames = self._names()
        return {n: ops.download(eng.pview[n]) for n in pnames}, {n: ops.download(eng.state[n]) for n in snames}

    def _repack(self, params, state):
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
            self._pack(params, state)
            self.stream.synchronize()

    def refresh(self):
        """(Re-)read the variables (the model's current ones, or the checkpoint's), fold the batch norms and re-pack the filters
        in place: captured programs stay valid."""
        self._repack(*self._variables())

    # ------------------------------------------------------------------------------------------------------------------------
    def _ensure_capacity(self, batch):
        """Buffers of one bucket, sized for the largest bucket run so far (smaller buckets use leading views).  Allocated with the
        object's stream current: the caching allocator ties a block to the stream it was allocated on."""
        if batch <= self._cap:
            return
        self.stream.synchronize()
        self._graphs = {}                              # they address the old buffers
        with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
            self._img = torch.zeros(batch, self.S, self.S, 3, device=self.dev)
            self._xin = None
            n_act = encoder_act_elems(self.spec, self.S, batch)
            self._act = [torch.zeros(n_act, dtype=self.dt, device=self.dev) for _ in range(2)]
            self._alloc(batch)
        self._cap = batch

    def _xin_for(self, batch):
        if self._xin is None or self._xin.shape[0] < batch:
            with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
                self._xin = torch.zeros(self._cap, self.S, self.S, 32, dtype=self.dt, device=self.dev)
        return self._xin[:batch]

    def _launch(self, key, program, ahead=False):
        """Issue the launches program() returns (those with a fn) on the current stream: one by one without use_graph, else as the
        graph cached under `key`, captured on a miss.  ahead=True only makes sure of the cache (a miss captures, with its
        synchronisation, and launches once; a hit and use_graph=False do nothing): what a caller does ahead of a clip's first frame."""
        if ahead and (not self.use_graph or key in self._graphs):
            return
        if not self.use_graph:
            for l in program():
                if l.fn is not None:
                    l.fn()
            return
        g = self._graphs.get(key)
        if g is None:
            prog = [l for l in program() if l.fn is not None]
            for l in prog:                 # warm-up outside capture (code-object loading, LDS attribute calls)
                l.fn()
            self.stream.synchronize()
            g = ops.Graph()
            g.capture_begin()
            for l in prog:
                l.fn()
            g.capture_end()
            self._graphs[key] = g
        g.launch()

    def _stage(self, count, bucket, images=None, boxes=None, packed=None):
        """The input rows of one bucket (current stream): _img[:count] filled, _img[count:bucket] zeroed.  images: a float batch
        [count, S, S, 3] (host or device), or a list of u8 photos resized on the GPU, with boxes (int32 [count, 5] rows over that list)
        cut and resized per box; or packed = (src, offs_d, hw_d, boxes_d), pack_u8's tensors with this bucket's count box rows.  Returns
        the packed tensors (None for a float batch)."""
        self._ensure_capacity(bucket)
        S, dst = self.S, self._img[:count]
        if packed is not None:
            ops.resize_crop_u8(packed[0], packed[1], packed[2], 3, (S, S), (0, 0), (S, S), dst, boxes=packed[3])
        elif isinstance(images, (list, tuple)):
            packed = stage_u8(images, dst, S, self.dev, boxes=boxes)
        else:
            self._stager.copy(dst, images, ('images', count))
        if count < bucket:
            self._img[count:bucket].zero_()
        return packed

    def _stage_rows(self, images, rows, start, count, bucket):
        """_stage of rows [start, start + count) of a call: of the images themselves (rows None), or of box rows int32 [n, 5] over u8
        photos: the photos these rows cut from, packed once each."""
        if rows is None:
            return self._stage(count, bucket, images[start:start + count])
        used, local = local_rows(rows[start:start + count])
        return self._stage(count, bucket, [images[i] for i in used], local)

    def _fork(self):
        """The object's stream waits for the caller's current stream, which is returned."""
        cur = torch.cuda.current_stream(self.dev)
        self.stream.wait_stream(cur)
        return cur

    def _join(self, cur, *record):
        """The caller's stream waits for the object's; the tensors in `record` (None skipped), allocated on the caller's stream and
        used on the object's, are made known to the allocator."""
        cur.wait_stream(self.stream)
        for t in record:
            if t is not None:
                t.record_stream(self.stream)

    @contextlib.contextmanager
    def _forked(self, *record):
        """with self._forked(tensors...): the body runs with the object's device and stream current, between _fork and _join."""
        cur = self._fork()
        with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
            yield cur
        self._join(cur, *record)


class LandmarkDetector(BucketRunner):
    """Unsupervised landmarks of a trained model: detect(images) -> mu f32 [N, K, 2], (y, x) in [-1, 1] (= the eval path's
    `gauss_yx`).  `model` is an IMMModel whose variables exist (trained, restored, or built once); the detector reads them,
    never writes them, and refresh() re-reads them after further training."""
    what = 'detector'

    def __init__(self, model, image_size=128, max_batch=256, use_graph=True):
        super(LandmarkDetector, self).__init__(model, image_size, max_batch, use_graph)

    @classmethod
    def from_checkpoint(cls, config, path, image_size=128, max_batch=256, dtype=torch.bfloat16, device=None, use_graph=True):
        """A detector straight from a checkpoint (`.pt` file or TensorFlow bundle prefix), without a training engine.
        config: the `model:` block of the experiment config (config.model)."""
        return cls._from_variables(config, read_checkpoint(path, int(config.n_filters)), image_size, max_batch, dtype, device,
                                   use_graph)

    # ------------------------------------------------------------------------------------------------------------------------
    def _setup(self, cfg, dtype, device, image_size, max_batch, use_graph):
        super(LandmarkDetector, self)._setup(cfg, dtype, device, image_size, max_batch, use_graph)
        K, He, C = self.K, self.He, 8 * self.nf
        if self.spec[0][0] != 7 or self.spec[0][1] != 3:
            raise NotImplementedError('first encoder layer must be 7x7 over RGB')
        self.ldh = ops.round_up(K, 4)
        # the one-launch pose head (imm_pose_head_fwd), under the engine's conditions; else the 1x1 convolution + soft-argmax pair
        self.fused_head = (C % 32 == 0 and (He * He) % 16 == 0 and 4 * (He * He * K + 2 * He * K + 2 * K) <= 158 * 1024 and
                           4 * ((2 + 2 * He) * K + 516) + He * He * ops.round_up(K, 32) * 2 <= 158 * 1024)
        with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
            # packed filters and folded biases (shared by every bucket)
            self.wt, self.bias = alloc_encoder_weights(self.spec, dtype, self.dev)
            self.kpad = [w.shape[1] for w in self.wt]
            self.wt_head = torch.zeros(ops.round_up(K, 128), ops.round_up(C, 32), dtype=dtype, device=self.dev)
            self.bias_head = torch.zeros(K, dtype=torch.float32, device=self.dev)
            # keypoints(): the regressor's W [2K, 2M] and b [2M] at fixed addresses (rewritten before each call's replays)
            self._kp_w = torch.zeros(2 * K * 2 * ops.MAX_KEYPOINTS, device=self.dev)
            self._kp_b = torch.zeros(2 * ops.MAX_KEYPOINTS, device=self.dev)
            # align(): F transposed [2K, 2 m3] at a fixed address (rewritten before each call's replays); the tps bases
            # [m3, So * So] are made on first use, per (template, So)
            self._al_ft = torch.zeros(2 * K * 2 * ops.MAX_ALIGN_M3, device=self.dev)
        self._al_basis = {}

    def _names(self):
        return pose_encoder_names(self.nf)

    def _pack(self, params, state):
        pack_folded_encoder(params, state, POSE_SCOPE, self.spec, self.wt, self.bias, self.dev)
        C = 8 * self.nf
        w_dev = torch.empty(1, 1, C, self.K, dtype=torch.float32, device=self.dev)
        ops.upload(w_dev, params[POSE_SCOPE + '/conv_1/w'], POSE_SCOPE + '/conv_1/w')
        rows, kpad = self.wt_head.shape
        ops.pack_weights(w_dev, self.wt_head, 0, 1, 1, C, self.K, C, rows, kpad)
        ops.upload(self.bias_head, params[POSE_SCOPE + '/conv_1/b'], POSE_SCOPE + '/conv_1/b')

    def _alloc(self, batch):
        K, He = self.K, self.He
        self._heat = torch.zeros(batch, He, He, self.ldh, device=self.dev)
        self._mu = torch.zeros(batch, K, 2, device=self.dev)
        self._py = torch.zeros(batch, He, K, device=self.dev)
        self._px = torch.zeros(batch, He, K, device=self.dev)
        self._geom = torch.zeros(batch, 4, device=self.dev)                        # keypoints(): (y0, x0, sy, sx) per row
        self._kp = torch.zeros(batch * ops.MAX_KEYPOINTS * 2, device=self.dev)     # keypoints(): [batch, M, 2]
        self._al_coef = torch.zeros(batch * ops.MAX_ALIGN_M3 * 2, device=self.dev)  # align(): [batch, m3, 2]

    def program(self, batch, u8=False, kp_m=None, align=None):
        """The launches of one bucket: [_Launch(tag, name, family, fn)].  tag: 'resize' | 'pack_image' | 'conv' | 'pose_head'
        (| 'softargmax' for heads the one-launch kernel does not serve); family: the conv kernel family (imm_conv2d_variant's,
        'first' for imm_conv_first).  kp_m: the program of keypoints() with M annotated points: the pose head with its keypoint
        epilogue (tag 'pose_head_kp').  align = (model, m3): the program of align(): detect()'s, then 'align_coeffs' (captured with
        it) and 'align_warp' (issued by align() with the call's pixels, like 'resize')."""
        if align is not None and kp_m is not None:
            raise ValueError('a program serves keypoints() or align(), not both')
        self._ensure_capacity(batch)
        B, S, dt = int(batch), self.S, self.dt
        prog = []
        if u8:
            prog.append(_Launch('resize', 'resize_crop_u8', 'resize', None))     # issued by detect() with the call's pixels
        enc, x, H, _ld = folded_encoder_program(POSE_SCOPE, self.spec, B, S, self._img[:B], self._act, self.wt, self.bias,
                                                self._xin_for, dt)
        prog += enc
        He, K, C = self.He, self.K, 8 * self.nf
        assert H == He
        heat, mu, py, px = self._heat[:B], self._mu[:B], self._py[:B], self._px[:B]
        mode = self.cfg.gauss_mode
        if kp_m is not None:
            if not self.fused_head:
                raise NotImplementedError('keypoints() needs the one-launch pose head (imm_pose_head_fwd), which does not serve '
                                          'this model (8 * n_filters = %d, heat map %dx%d, K = %d)' % (C, He, He, K))
            M = int(kp_m)
            kw, kb = self._kp_w[:2 * K * 2 * M].view(2 * K, 2 * M), self._kp_b[:2 * M]
            geom, kp = self._geom[:B], self._kp[:B * M * 2].view(B, M, 2)
            prog.append(_Launch('pose_head_kp', POSE_SCOPE + '/conv_1', 'pose_head', lambda: ops.pose_head_fwd(
                x, C, C, self.wt_head, self.bias_head, B, He, He, K, self.inv_std, 16, heat, self.ldh, mu, py, px, None, K, dt, mode,
                keypoints=ops.keypoint_desc(kw, kb, geom, kp, self.S))))
        elif self.fused_head:
            prog.append(_Launch('pose_head', POSE_SCOPE + '/conv_1', 'pose_head', lambda: ops.pose_head_fwd(
                x, C, C, self.wt_head, self.bias_head, B, He, He, K, self.inv_std, 16, heat, self.ldh, mu, py, px, None, K, dt, mode)))
        else:
            d = ops.fwd_desc(B, He, He, C, C, K, self.ldh, 1, 1, L.CONV_BIAS | L.CONV_OUT_F32)
            prog.append(_Launch('conv', POSE_SCOPE + '/conv_1', ops.conv2d_variant(d, dt)[0],
                                lambda: ops.conv2d(d, x, self.wt_head, self.bias_head, heat)))
            prog.append(_Launch('softargmax', POSE_SCOPE + '/softargmax', 'softargmax', lambda: ops.softargmax_gauss_fwd(
                heat, self.ldh, B, He, He, K, self.inv_std, 16, mu, py, px, None, K, dt, mode)))
        if align is not None:
            m3 = int(align[1])
            if m3 != (K + 3 if align[0] == 'tps' else 3):
                raise ValueError('align = (model, m3): %r has m3 = %d at K = %d' % (align[0], K + 3 if align[0] == 'tps' else 3, K))
            ft, coef = self._al_ft[:2 * K * 2 * m3].view(2 * K, 2 * m3), self._al_coef[:B * m3 * 2].view(B, m3, 2)
            prog.append(_Launch('align_coeffs', 'align/coeffs', 'align', lambda: ops.align_coeffs(mu, ft, K, m3, coef)))
            prog.append(_Launch('align_warp', 'align/warp', 'align', None))     # issued by align() with the call's pixels
        return prog

    def _keyed(self, batch, kp_m=None, align=None):
        key = batch if kp_m is None else (batch, int(kp_m))
        if align is not None:
            key = (batch, 'align', int(align[1]))
        return key, lambda: self.program(batch, kp_m=kp_m, align=align)

    def _run(self, batch, kp_m=None, align=None):
        """Issue the (graph of the) program of bucket `batch` (with the keypoint epilogue of M = kp_m points, or with align()'s
        coefficient launch) on the detector's stream."""
        self._launch(*self._keyed(batch, kp_m, align))

    def _capture(self, batch, kp_m=None):
        """Make sure _run(batch, kp_m) finds its graph captured (_launch, ahead=True)."""
        self._launch(*self._keyed(batch, kp_m), ahead=True)

    # ------------------------------------------------------------------------------------------------------------------------
    def detect(self, images, heatmaps=False):
        """images: NHWC float [N, S, S, 3] with values in [0, 255] (host or device), or a list of u8 HWC arrays of any sizes
        (resized to S x S on the GPU).  Returns mu f32 [N, K, 2] on the detector's device, and with heatmaps=True also the pose
        head's heat maps f32 [N, S/8, S/8, K]."""
        images, _u8 = as_image_batch(images, self.S)
        N, K, He = len(images), self.K, self.He
        mu_out = torch.empty(N, K, 2, device=self.dev)
        heat_out = torch.empty(N, He, He, K, device=self.dev) if heatmaps else None
        with self._forked():
            for start, count, bucket in plan_buckets(N, self.max_batch):
                self._stage_rows(images, None, start, count, bucket)
                self._run(bucket)
                mu_out[start:start + count].copy_(self._mu[:count])
                if heatmaps:
                    heat_out[start:start + count].copy_(self._heat[:count, ..., :K])
        return (mu_out, heat_out) if heatmaps else mu_out

    def keypoints(self, images, regressor, boxes=None, return_mu=False):
        """The regressor's M annotated points in source pixels: f32 [n, M, 2] (y, x) on the detector's device, one row per box
        (per image without boxes), and with return_mu=True also the landmarks mu f32 [n, K, 2] of the same rows.
        images: as detect() takes them.  regressor: a keypoints.LandmarkRegressor fitted for this detector's K and S.
        boxes: only with a list of u8 arrays: rows (image, y0, x0, y1, x1) or one (y0, x0, y1, x1) per image, half-open, in source
        pixels (keypoints.check_boxes); each box is cut from its image with zero padding where it leaves it and resized to S x S on
        the GPU.  Without boxes, u8 images are resized whole (the points scale back by h / S, w / S) and a tensor batch is already
        the S x S frame."""
        regressor.check(self.K, self.S)
        w, b = regressor.epilogue_weights()
        M = regressor.M
        images, _u8, rows, geom = photo_rows(images, boxes, self.S)
        N, K = len(geom), self.K
        kp_out = torch.empty(N, M, 2, device=self.dev)
        mu_out = torch.empty(N, K, 2, device=self.dev) if return_mu else None
        with self._forked():
            self._stager.copy(self._kp_w[:w.size], torch.from_numpy(w.reshape(-1)), ('kp_w', M))
            self._stager.copy(self._kp_b[:b.size], torch.from_numpy(b), ('kp_b', M))
            for start, count, bucket in plan_buckets(N, self.max_batch):
                self._stage_rows(images, rows, start, count, bucket)
                self._stager.copy(self._geom[:count], torch.from_numpy(geom[start:start + count]), ('geom', count))
                self._run(bucket, M)
                kp_out[start:start + count].copy_(self._kp[:count * M * 2].view(count, M, 2))
                if return_mu:
                    mu_out[start:start + count].copy_(self._mu[:count])
        return (kp_out, mu_out) if return_mu else kp_out

    def _align_basis(self, template, model, So):
        """The tps basis f32 [m3, So * So] of a template on the device (made once per template and output size); None for the
        similarity and affine models, which read none."""
        if model != 'tps':
            return None
        key = (template.points.tobytes(), int(So))
        if key not in self._al_basis:
            if len(self._al_basis) >= 8:                                   # a caller cycling through templates: drop the oldest
                self._al_basis.pop(next(iter(self._al_basis)))
            self._al_basis[key] = ops.to_device_pinned(np.ascontiguousarray(template.basis('tps', So), dtype=np.float32), self.dev)
        return self._al_basis[key]

    def landmarks(self, images, boxes=None):
        """detect() per face box: mu f32 [n, K, 2] of the rows keypoints() and align() would work on (one per box, cut with zero
        padding and resized to S x S on the GPU; one per image without boxes)."""
        images, u8, rows = photo_boxes(images, boxes, self.S)
        if not u8:
            return self.detect(images)
        N = len(rows)
        mu_out = torch.empty(N, self.K, 2, device=self.dev)
        with self._forked():
            for start, count, bucket in plan_buckets(N, self.max_batch):
                self._stage_rows(images, rows, start, count, bucket)
                self._run(bucket)
                mu_out[start:start + count].copy_(self._mu[:count])
        return mu_out

    def quality(self, images, boxes=None, template=None, gate=None):
        """How far every row's landmarks deserve trust: a quality.LandmarkQuality (mu f32 [n, K, 2], spread f32 [n, K], score f32 [n, 2] =
        (mean spread, shape residual), flags int32 [n], and the soft-argmax marginals py, px f32 [n, S/8, K]) on the detector's device,
        one row per box (per image without boxes).  images, boxes: as keypoints() takes them.  template: an alignment.LandmarkTemplate
        of this detector's K and S, the reference shape of the residual (taken on the landmarks themselves: the template lives in the
        S x S frame); without one the residual is 0.  gate: a quality.QualityGate whose thresholds set the flags; without one only a
        NaN score sets a flag.  Stills are scored, never blanked: mu is detect()'s.
        Per bucket: detect()'s program, then imm_landmark_scores (include/imm_score.h) on the buffers it left, then device copies.
        Nobody has measured how well these scores tell a face from a non-face: see quality.py."""
        from . import quality as QL
        QL.check_gate(gate, self.K, self.S)
        if template is not None:
            template.check(self.K, self.S)
        images, _u8, rows, geom = photo_rows(images, boxes, self.S)
        N, K, He = len(geom), self.K, self.He
        held = _Held(self.dev)
        with torch.cuda.device(self.dev):
            ref = None if template is None else held.up(np.ascontiguousarray(template.points, dtype=np.float64))
            mu, spread, score, flags = held.empty(N, K, 2), held.empty(N, K), held.empty(N, 2), held.empty(N, dtype=torch.int32)
            py, px = held.empty(N, He, K), held.empty(N, He, K)
        with self._forked(*held):
            for start, count, bucket in plan_buckets(N, self.max_batch):
                self._stage_rows(images, rows, start, count, bucket)
                self._run(bucket)
                sl = slice(start, start + count)
                ops.landmark_scores(self._py[:count], self._px[:count], self._mu[:count], None, ref, 0, self.S,
                                    None if gate is None else gate.max_spread, None if gate is None else gate.max_residual, 0,
                                    spread[sl], score[sl], flags[sl], None)
                mu[sl].copy_(self._mu[:count])
                py[sl].copy_(self._py[:count])
                px[sl].copy_(self._px[:count])
        return QL.LandmarkQuality(mu, spread, score, flags, py, px, self.S)

    def track(self, frames, boxes, regressor=None, box_smooth=0.5, one_euro=OneEuro(), fps=25.0, chunk_frames=32):
        """The faces of a clip followed from its first frame: a tracking.Track (mu, points, points_smooth [T, F, K, 2], boxes int32
        [T, F, 4], flags [T, F], keypoints [T, F, M, 2] with a regressor) on the detector's device.
        frames: a list of T u8 HWC arrays of any sizes.  boxes: the faces of frames[0], rows (0, y0, x0, y1, x1) or (y0, x0, y1, x1),
        as keypoints.check_boxes takes them; at most max_batch of them.  box_smooth in (0, 1]: the weight of a frame's measurement in
        the box filter.  one_euro: a tracking.OneEuro (the default: OneEuro()), or None for points_smooth == points.  fps: the clip's
        frame rate (the filter's time step).  chunk_frames: frames packed and uploaded at a time.
        With a quality gate the same clip is tracked by tracker(..., gate=gate).track(frames, boxes, chunk_frames).
        Per frame, on the detector's stream: imm_resize_crop_u8 with the box rows the frame before left in device memory, the bucket's
        captured program (with the keypoint epilogue, given a regressor), imm_track_step (include/imm_track.h) and a device copy of the
        landmarks.  Between the first and the last frame's launches nothing is copied to the host and the stream is not synchronised."""
        from . import tracking as TR
        frames, rows, beta, _consts, chunk = TR.plan_track(frames, boxes, self.max_batch, box_smooth, one_euro, fps, chunk_frames)
        return TR.FaceTracker(self, regressor, beta, one_euro, fps, capacity=len(frames)).run(frames, rows, chunk)

    def tracker(self, regressor=None, box_smooth=0.5, one_euro=OneEuro(), fps=25.0, gate=None):
        """A tracking.FaceTracker for live input: .start(frame, boxes), .step(frame), .result() -> the Track of the frames seen so far.
        The launches of track(), with one-frame uploads; .track(frames, boxes, chunk_frames) runs a whole clip as track() does.
        gate: a quality.QualityGate, or None.  With one, every frame's faces are scored (Track.spread, .score, .qflags) and a face that
        fails the gate's thresholds on a frame after the first is lost on that frame (Track.unsure, Track.lost): its box and filters
        stay, its points are NaN.  No default thresholds exist: a gate is fitted on faces known to be good (quality.QualityGate.fit)."""
        from . import tracking as TR
        return TR.FaceTracker(self, regressor, box_smooth, one_euro, fps, gate=gate)

    def align(self, images, template, boxes=None, model='similarity', lam=0.0, out_size=None, return_transform=False, _packed=None):
        """Every face warped so that its landmarks land on the template: f32 [n, So, So, 3] in [0, 255] on the detector's device, one
        row per box (per image without boxes); with return_transform=True also an alignment.Alignment (coef, geom, mu, to_source,
        to_aligned).  images, boxes: as keypoints() takes them.  template: an alignment.LandmarkTemplate of this detector's K and S.
        model: 'similarity' | 'affine' | 'tps' (lam >= 0: its smoothing).  out_size So defaults to S.
        The landmarks come from detect()'s program on the S x S crop of each box; the backward map's coefficients are one more launch
        in that program (imm_align_coeffs) and the photo is then sampled ONCE, straight from the packed u8 pixels, through the map and
        the box geometry (imm_align_warp_u8) - the S x S crop is not resampled.  A tensor batch [N, S, S, 3] is its own source: the
        staged f32 copy the detector reads is sampled in place of u8 photos, geometry (0, 0, 1, 1).
        _packed (internal; ImageGenerator.repose): pack_u8(images, device, rows) of exactly these u8 images and box rows, made by a
        caller that needs the packed photos itself; the buckets then read that one buffer instead of packing their own photos."""
        from . import alignment as AL
        lam = AL.check_model(model, lam)
        template.check(self.K, self.S)
        So = self.S if out_size is None else int(out_size)
        if So < 1 or So > 8192:
            raise ValueError('out_size must be in [1, 8192], got %d' % So)
        K, m3 = self.K, AL.n_basis(model, self.K)
        ft = np.ascontiguousarray(template.fit_matrix(model, lam).T, dtype=np.float32)             # [2K, 2 m3]
        images, u8, rows, geom = photo_rows(images, boxes, self.S)
        N = len(geom)
        out = torch.empty(N, So, So, 3, device=self.dev)
        coef_out = torch.empty(N, m3, 2, device=self.dev) if return_transform else None
        mu_out = torch.empty(N, K, 2, device=self.dev) if return_transform else None
        with self._forked():
            basis = self._align_basis(template, model, So)
            self._stager.copy(self._al_ft[:ft.size], torch.from_numpy(ft.reshape(-1)), ('al_ft', m3))
            for start, count, bucket in plan_buckets(N, self.max_batch):
                if u8 and _packed is not None:
                    packed = self._stage(count, bucket, packed=tuple(_packed[:3]) + (_packed[3][start:start + count],))
                else:
                    packed = self._stage_rows(images, rows, start, count, bucket)
                src, offs_d, hw_d, boxes_d = packed if u8 else (self._img[:count], None, None, None)
                self._stager.copy(self._geom[:count], torch.from_numpy(geom[start:start + count]), ('geom', count))
                self._run(bucket, align=(model, m3))
                coef = self._al_coef[:bucket * m3 * 2].view(bucket, m3, 2)[:count]
                ops.align_warp_u8(src, offs_d, hw_d, boxes_d, self._geom[:count], coef, basis, self.S, out[start:start + count])
                if return_transform:
                    coef_out[start:start + count].copy_(coef)
                    mu_out[start:start + count].copy_(self._mu[:count])
        if return_transform:
            return out, AL.Alignment(coef_out, ops.to_device_pinned(geom, self.dev), mu_out, model, lam, template, So, rows)
        return out

    def warp(self, photos, poses, boxes=None, pose_boxes=None, feather=0.125, anchors=2, lam=0.0, strength=1.0, return_transform=False):
        """The photos with every box's face re-posed from the photo's OWN pixels: a list of u8 device tensors [h_i, w_i, 3], one per
        photo, views of one packed buffer (as ImageGenerator.repose returns them); nothing is rendered.
        photos, boxes, poses, pose_boxes: as ImageGenerator.repose takes them (a list of u8 arrays; n box rows, by default one
        whole-photo box per photo; landmarks f32 [n, K, 2] or [1, K, 2] in the box frame, or a list of u8 pose photos whose landmarks
        are detector.landmarks(poses, pose_boxes)).  Per row a thin-plate spline is fitted on the device (imm_warp_fit) that carries the
        target landmarks back to the face's own landmarks and `anchors` points per side of the box border (corners included; 0: none)
        to themselves; every pixel of the box then takes the original photo's value at the place the spline sends it to, bilinearly,
        faded into the photo over `feather` of the box side (imm_warp_u8; include/imm_warp.h states the rule).  lam >= 0 smooths the
        spline (0: it interpolates), strength scales the motion (0: the photo itself; 1: the pose).  K + 4 * anchors must lie in
        [3, 80]; host poses whose control points lie closer than 1e-6 are refused.  Rows are applied in row order, each sampling the ORIGINAL pixels: an overlapping later box blends over an earlier
        one.  A row without a usable fit (coincident control points, a landmark that is not finite) leaves its box alone.
        Per bucket: imm_resize_crop_u8 from the original pixels, the captured pose program, imm_warp_fit reading the pose head's
        landmarks in place, imm_warp_u8, all on the detector's stream; nothing returns to the host.
        return_transform=True: (photos, a warping.PhotoWarp: coef, ctrl, rows, mu, poses, flags, to_source)."""
        from . import warping as WP
        from .generation import PasteSetup
        K = self.K
        photos, rows, pose, feather, m, lam, strength, M = WP.plan_warp(photos, poses, boxes, pose_boxes, feather, K, anchors, lam, strength)
        n = len(rows)
        held = _Held(self.dev)
        lm = held.keep(pose_landmarks(self, pose, n).contiguous())
        buckets = plan_buckets(n, self.max_batch)
        ps = PasteSetup(photos, rows, buckets, feather, self.dev)                   # all photos, once per call
        held.keep(*ps.tensors())
        with torch.cuda.device(self.dev):
            anchors_d = held.up(WP.warp_anchors(m).astype(np.float32)) if m else None
            coef, ctrl = held.empty(n, M + 3, 2), held.empty(n, M, 2)
            flags = held.empty(n, dtype=torch.int32)
            mu_out = held.empty(n, K, 2) if return_transform else None
        with self._forked(*held):
            for start, count, bucket in buckets:
                part = slice(start, start + count)
                self._stage(count, bucket, packed=ps.packed(part))
                self._run(bucket)
                ops.warp_fit(lm[part], self._mu[:count], anchors_d, strength, lam, coef[part], ctrl[part], flags[part])
                ops.warp_u8(ps.src, ps.canvas, ps.offs_d, ps.hw_d, ps.boxes_d[part], ps.links_d[part], ps.ramp_d[part], ctrl[part],
                            coef[part], ps.max_pixels(part))
                if return_transform:
                    mu_out[part].copy_(self._mu[:count])
        out = unpack_u8(ps.canvas, photos)
        if return_transform:
            return out, WP.PhotoWarp(coef, ctrl, rows, mu_out, lm, flags, strength, lam, m)
        return out

    def morph(self, photos, donors, boxes=None, donor_boxes=None, shape=0.5, texture=None, feather=0.125, anchors=2, lam=0.0,
              landmarks=None, donor_landmarks=None, return_transform=False, colour=0.0, max_gain=2.0, mask=None, grow=1.25,
              mask_feather=0.1, seamless=0.0, ring=128):
        """The photos with every box's face blended with a donor's face, in shape and in texture, from the pixels of the two
        photographs: a list of u8 device tensors [h_i, w_i, 3], one per photo, views of one packed buffer (what warp returns); nothing
        is rendered.
        photos, boxes: as warp takes them.  donors, donor_boxes: the donor faces in the same forms (a list of u8 arrays; box rows, by
        default one whole-photo box per donor photo): one donor row per face, or ONE for all.  shape and texture: a number or one per
        row, in [0, 1].  shape moves the landmarks from the face's own (0) to the donor's (1), each in the frame of its box; texture
        mixes the pixels from the face's own (0) to the donor's (1); texture=None: texture = shape, the morph at that point.  shape = 0,
        texture = 1 swaps the donor's face in, in place; texture = 0 is warp towards the blended pose.  feather, anchors, lam: as warp
        takes them.  landmarks, donor_landmarks: f32 [n, K, 2], the faces' own and the donors' landmarks where the caller has them
        (annotated, or from an earlier call); that side's pose program is then skipped.
        Per row the blended landmarks p = (1 - shape) mu + shape mu_donor and the anchors are the control points of two splines fitted by
        ONE imm_warp_fit launch: p -> mu in the face's box, p -> mu_donor in the donor's box.  Every pixel of the box takes the original
        photo's value at the first place and the donor photo's value at the second, bilinearly, mixed by texture and faded into the photo
        (imm_morph_u8; include/imm_morph.h states the rule).  Rows are applied in row order.  A row without a usable fit on either side
        leaves its box alone.
        Both photo lists are packed and uploaded once; the donors' landmarks are detector.landmarks(donors, donor_boxes).  Per bucket:
        imm_resize_crop_u8 from the original pixels and the captured pose program (unless landmarks is given), imm_morph_poses,
        imm_warp_fit over twice the rows, imm_morph_u8, all on the detector's stream; nothing returns to the host.
        colour: a number or one per row in [0, 1], how far the donor's pixels take the face's tone (0, the default: not at all, today's
        launches and bytes; 1: the donor region's mean and spread per channel become the face region's).  The regions are the ellipses
        inscribed in the two boxes as they lie in their photographs; the ratio of the spreads is kept in [1 / max_gain, max_gain]
        (max_gain finite, >= 1).  With any colour > 0, once per call in front of the buckets: imm_colour_stats_u8 over the faces' rows
        and over the donors' rows, imm_colour_gain; and per bucket imm_morph_colour_u8 in place of imm_morph_u8 (include/imm_colour.h
        states the rule).
        mask: None (the default: every pixel of the box is blended, today's launches and bytes) or 'hull': only the face is pasted.
        The convex hull of the row's blended landmarks, grown about their centroid by grow (a number or one per row in (0, 16]) and
        softened inwards over mask_feather * min(H, W) pixels (a number or one per row in [0, 1]; at least one pixel), multiplies the
        box's edge ramp, and pixels outside it skip the spline.  Per bucket imm_hull_fit runs behind imm_morph_poses, reading the blended
        landmarks in place, and imm_morph_hull_u8 takes the place of imm_morph_u8 / imm_morph_colour_u8 (include/imm_hull.h states the
        rule).
        seamless: a number or one per row in [0, 1] (0, the default: today's launches and bytes); any seamless > 0 needs mask='hull'.
        The donor's pixels keep their detail and take a smooth correction that carries them onto the photo's own values on the outline
        of the mask: at ring (an int in [16, 256], one for the call) samples of the outline the photo minus the morph's mix, and per
        pixel the mean of those differences weighed by the pixel's mean-value coordinates, times seamless.  Per bucket imm_seam_fit runs
        behind the spline fit and imm_morph_seam_u8 takes the place of imm_morph_hull_u8 (include/imm_seam.h states the rule).
        return_transform=True: (photos, a morphing.PhotoMorph: coef_a, coef_b, ctrl, rows, donor_rows, mu, donor_mu, poses, flags,
        to_source, to_donor, colour_gain, colour_flags, hull_edges, hull_flags, hull_weight, seam_ring, seam_diff, seam_flags,
        seam_field)."""
        from . import morphing as MP
        from . import warping as WP
        from .generation import PasteSetup, box_areas
        K = self.K
        plan = MP.plan_morph(photos, donors, boxes, donor_boxes, shape, texture, feather, K, anchors, lam, landmarks, donor_landmarks, colour,
                             max_gain, mask, grow, mask_feather, seamless, ring)
        photos, rows, drows, m, lam, M = plan.photos, plan.rows, plan.donor_rows, plan.anchors, plan.lam, plan.M
        n = len(rows)
        matched, hull, seam = bool(plan.colour.any()), plan.mask == 'hull', bool(plan.seamless.any())
        held = _Held(self.dev)                                                      # what _forked records: every tensor made below
        lm_b = held.keep(pose_landmarks(self, ('photos', plan.donors, plan.donor_rows_given) if plan.donor_landmarks is None else
                                        ('landmarks', plan.donor_landmarks), n).contiguous())
        lm_a = None if plan.landmarks is None else held.keep(plan.landmarks.to(device=self.dev, dtype=torch.float32).contiguous())
        buckets = plan_buckets(n, self.max_batch)
        ps = PasteSetup(photos, rows, buckets, plan.feather, self.dev)              # all photos, once per call
        held.keep(*ps.tensors())
        extra = {}                                                                  # morph_paste's optional tensors, one row each
        with torch.cuda.device(self.dev):
            don, doffs_d, dhw_d, dboxes_d = held.keep(*pack_u8(plan.donors, self.dev, drows))      # all donor photos, once per call
            shape_d, texture_d = held.up(plan.shape), held.up(plan.texture)
            anchors_d = held.up(WP.warp_anchors(m).astype(np.float32)) if m else None
            coef_a, coef_b, ctrl = held.empty(n, M + 3, 2), held.empty(n, M + 3, 2), held.empty(n, M, 2)
            flags = held.empty(n, dtype=torch.int32)
            poses = held.empty(n, K, 2) if return_transform else None
            mu_out = held.empty(n, K, 2) if return_transform and lm_a is None else None
            # one bucket's scratch: the inputs and outputs of the fit over 2 * count rows
            B = max(count for _s, count, _b in buckets)
            poses2, mu2 = held.empty(2 * B * K * 2), held.empty(2 * B * K * 2)
            coef2, ctrl2 = held.empty(2 * B * (M + 3) * 2), held.empty(2 * B * M * 2)
            flags2 = held.empty(2 * B, dtype=torch.int32)
            cflags, hflags, sflags = (held.empty(n, dtype=torch.int32) if on else None for on in (matched, hull, seam))
            if matched:
                colour_d, sums2 = held.up(plan.colour), held.empty(2, n, 7, dtype=torch.int64)
                extra['gain'] = held.empty(n, 3, 2)
            if hull:
                grow_d, extra['inv_soft'], extra['edges'] = held.up(plan.grow), held.up(plan.inv_soft), held.empty(n, K, 3)
            if seam:
                extra['seamless'], dirs_d = held.up(plan.seamless), held.up(MP.seam_dirs(plan.ring))
                extra['ring'], extra['diff'] = held.empty(n, plan.ring, 2), held.empty(n, plan.ring, 3)
        with self._forked(*held):
            if matched:                                                             # once per call, all rows
                ops.colour_stats_u8(ps.src, ps.offs_d, ps.hw_d, ps.boxes_d, int(ps.area.max()), sums2[0])
                ops.colour_stats_u8(don, doffs_d, dhw_d, dboxes_d, int(box_areas(drows).max()), sums2[1])
                ops.colour_gain(sums2[0], sums2[1], colour_d, plan.max_gain, extra['gain'], cflags)
            for start, count, bucket in buckets:
                part = slice(start, start + count)
                opt = {k: t[part] for k, t in extra.items()}
                if lm_a is None:
                    self._stage(count, bucket, packed=ps.packed(part))
                    self._run(bucket)
                    own = self._mu[:count]
                else:
                    own = lm_a[part]
                p2, m2 = poses2[:2 * count * K * 2].view(2, count, K, 2), mu2[:2 * count * K * 2].view(2, count, K, 2)
                c2, t2 = coef2[:2 * count * (M + 3) * 2].view(2, count, M + 3, 2), ctrl2[:2 * count * M * 2].view(2, count, M, 2)
                f2 = flags2[:2 * count].view(2, count)
                ops.morph_poses(own, lm_b[part], shape_d[part], p2, m2)
                if hull:                                                            # the blended landmarks, read in place
                    ops.hull_fit(p2[0], ps.boxes_d[part], grow_d[part], opt['edges'], hflags[part])
                ops.warp_fit(p2.view(2 * count, K, 2), m2.view(2 * count, K, 2), anchors_d, 1.0, lam, c2.view(2 * count, M + 3, 2),
                             t2.view(2 * count, M, 2), f2.view(2 * count))
                coef_a[part].copy_(c2[0])
                coef_b[part].copy_(c2[1])
                ctrl[part].copy_(t2[0])
                torch.bitwise_or(f2[0], f2[1], out=flags[part])
                if seam:
                    ops.seam_fit(p2[0], ps.boxes_d[part], grow_d[part], opt['edges'], hflags[part], dirs_d, ps.src, ps.offs_d, ps.hw_d, don,
                                 doffs_d, dhw_d, dboxes_d[part], texture_d[part], t2[0], c2[0], c2[1], opt.get('gain'), opt['ring'],
                                 opt['diff'], sflags[part])
                ops.morph_paste(ps.src, ps.canvas, ps.offs_d, ps.hw_d, don, doffs_d, dhw_d, ps.boxes_d[part], dboxes_d[part], ps.links_d[part],
                                ps.ramp_d[part], texture_d[part], t2[0], c2[0], c2[1], ps.max_pixels(part), **opt)
                if return_transform:
                    poses[part].copy_(p2[0])
                    if mu_out is not None:
                        mu_out[part].copy_(own)
        out = unpack_u8(ps.canvas, photos)
        if return_transform:
            return out, MP.PhotoMorph(
                coef_a=coef_a, coef_b=coef_b, ctrl=ctrl, rows=rows, donor_rows=drows, mu=mu_out if lm_a is None else lm_a, donor_mu=lm_b,
                poses=poses, flags=flags, shape=plan.shape, texture=plan.texture, lam=lam, anchors=m, colour=plan.colour,
                max_gain=plan.max_gain, colour_gain=extra.get('gain'), colour_flags=cflags, mask=plan.mask,
                grow=plan.grow if hull else None, mask_feather=plan.mask_feather if hull else None, inv_soft=plan.inv_soft if hull else None,
                hull_edges=extra.get('edges'), hull_flags=hflags, seamless=plan.seamless if seam else None,
                ring=plan.ring if seam else None, seam_ring=extra.get('ring'), seam_diff=extra.get('diff'), seam_flags=sflags)
        return out

    def morph_clip(self, frames, boxes, donors, donor_boxes=None, shape=0.0, texture=1.0, feather=0.125, anchors=2, lam=0.0,
                   donor_landmarks=None, colour=0.0, max_gain=2.0, mask=None, grow=1.25, mask_feather=0.1, seamless=0.0, ring=128,
                   smooth=True, colour_smooth=0.25, seam_smooth=0.25, box_smooth=0.5, one_euro=OneEuro(), fps=25.0, chunk_frames=32,
                   gate=None):
        """A donor's face follows a tracked face through a clip: track() and morph() joined on the device, a clip.ClipMorph (frames,
        track, own, fit_flags, colour_gain, colour_flags, hull_flags, seam_diff, seam_flags).
        frames, boxes, box_smooth, one_euro, fps, chunk_frames: exactly as track takes them; boxes are the F faces of frames[0], at most
        max_batch of them.  donors, donor_boxes, donor_landmarks: one donor row per face, or ONE for all, in morph's forms.  shape,
        texture, feather, anchors, lam, colour, max_gain, mask, grow, mask_feather, seamless, ring: as morph takes them, a number or
        one per face, with morph's refusals; the defaults shape = 0, texture = 1 swap the donor's face in, in place.
        smooth=True: the faces' own landmarks are the tracker's One-Euro points (Track.points_smooth) brought back into the frame of
        each frame's box; False: the pose head's mu.  colour_smooth and seam_smooth in (0, 1]: the weight of a frame's colour gain and
        of its membrane differences in a first-order filter, s <- s + a (x - s), box_smooth's convention; 1 means no filter, and the
        filter's launch is then not issued.  The defaults of 0.25 are by analogy with box_smooth: nobody has tuned them on footage.
        A face the tracker lost on a frame (Track.lost) is not pasted on that frame: the frame keeps its pixels there.  gate: a
        quality.QualityGate handed to the tracker, or None: a face that fails it on a frame is lost there (ClipMorph.track.unsure).
        Once per call the donors are packed and uploaded, their landmarks detected (unless given) and their colour sums taken; per chunk
        the frames are uploaded and copied into a canvas on the device; per frame the tracker's launches, imm_clip_rows
        (include/imm_clip.h) and morph's chain run on the detector's stream with the box rows the frame before left in device memory.
        Between the first and the last frame's launches nothing is copied to the host and the stream is not synchronised."""
        from . import clip as CL
        plan = CL.plan_clip(frames, boxes, donors, donor_boxes, shape, texture, feather, self.K, anchors, lam, donor_landmarks, colour, max_gain,
                            mask, grow, mask_feather, seamless, ring, smooth, colour_smooth, seam_smooth, box_smooth, one_euro, fps,
                            chunk_frames, self.max_batch, gate)
        return CL.run(self, plan)

    def redact(self, photos, boxes=None, mode='pixelate', blocks=8, mask=None, grow=1.25, mask_feather=0.1, feather=0.0, landmarks=None,
               return_transform=False):
        """The photos with every box's face made unreadable: a list of u8 device tensors [h_i, w_i, 3], one per photo, views of one
        packed buffer (what warp returns).  photos, boxes: as warp takes them.  The box is cut into square cells, at most `blocks` (an
        int in [1, 64]) along its longer side, every cell takes the mean of the ORIGINAL pixels it covers, and the box is pasted over
        with those means (mode='pixelate', a mosaic) or with their bilinear interpolation (mode='smooth', a blur), faded into the photo
        over `feather` of the box side (include/imm_redact.h states the rule).  Rows are applied in row order.
        mask: None (the default: the whole box) or 'hull': only the convex hull of the face's landmarks, grown by `grow` and softened
        inwards over mask_feather * min(H, W) pixels, as morph takes them.  landmarks: f32 [n, K, 2] where the caller has them; the pose
        program is then skipped.  Redaction FAILS CLOSED: a row whose hull is degenerate or whose landmarks are not finite (they are not
        refused) is redacted over its WHOLE box, where morph would leave it alone.  feather=0 and mask=None are the defaults because the
        hard, whole box is the conservative reading; nobody has measured how recognisable a face stays at any setting, and no anonymity
        is claimed.
        Per bucket, on the detector's stream, nothing returning to the host: with mask=None imm_redact_cells_u8 and imm_redact_u8 and
        NO pose program; with mask='hull' imm_resize_crop_u8 and the captured pose program (unless landmarks is given), imm_hull_fit
        reading the pose head's landmarks in place, then the same two.
        return_transform=True: (photos, a redaction.PhotoRedaction: rows, cells, cell, grid, mode, blocks, mu, hull_edges, hull_flags,
        inv_soft, weight)."""
        from . import redaction as RD
        from .generation import PasteSetup
        K = self.K
        plan = RD.plan_redact(photos, boxes, K, mode, blocks, mask, grow, mask_feather, feather, landmarks)
        photos, rows, nb, hull = plan.photos, plan.rows, plan.blocks, plan.mask == 'hull'
        n, code = len(rows), RD.MODES[plan.mode]
        held = _Held(self.dev)
        lm = None if plan.landmarks is None or not hull else held.keep(plan.landmarks.to(device=self.dev, dtype=torch.float32).contiguous())
        buckets = plan_buckets(n, self.max_batch)
        ps = PasteSetup(photos, rows, buckets, plan.feather, self.dev)              # all photos, once per call
        held.keep(*ps.tensors())
        extra = {}                                                                  # redact_u8's optional tensors, one row each
        with torch.cuda.device(self.dev):
            cells = held.empty(n, nb * nb * 3, dtype=torch.uint8)
            mu_out = None
            if hull:
                grow_d = held.up(plan.grow)
                extra = dict(edges=held.empty(n, K, 3), inv_soft=held.up(plan.inv_soft), hull_flags=held.empty(n, dtype=torch.int32))
                mu_out = held.empty(n, K, 2) if return_transform and lm is None else None
        with self._forked(*held):
            for start, count, bucket in buckets:
                part = slice(start, start + count)
                opt = {k: t[part] for k, t in extra.items()}
                if hull:
                    if lm is None:
                        self._stage(count, bucket, packed=ps.packed(part))
                        self._run(bucket)
                        own = self._mu[:count]
                    else:
                        own = lm[part]
                    ops.hull_fit(own, ps.boxes_d[part], grow_d[part], opt['edges'], opt['hull_flags'])
                    if mu_out is not None:
                        mu_out[part].copy_(own)
                ops.redact_cells_u8(ps.src, ps.offs_d, ps.hw_d, ps.boxes_d[part], nb, cells[part])
                ops.redact_u8(ps.canvas, ps.offs_d, ps.hw_d, ps.boxes_d[part], ps.links_d[part], ps.ramp_d[part], cells[part], nb, code,
                              ps.max_pixels(part), **opt)
        out = unpack_u8(ps.canvas, photos)
        if return_transform:
            return out, RD.PhotoRedaction(rows, cells, plan.mode, nb, plan.feather, mu=(mu_out if lm is None else lm) if hull else None,
                                          hull_edges=extra.get('edges'), hull_flags=extra.get('hull_flags'),
                                          inv_soft=plan.inv_soft if hull else None)
        return out

    def redact_clip(self, frames, boxes, mode='pixelate', blocks=8, mask=None, grow=1.25, mask_feather=0.1, feather=0.0, smooth=True,
                    box_smooth=0.5, one_euro=OneEuro(), fps=25.0, chunk_frames=32, gate=None):
        """The faces of a clip followed from its first frame and redacted on every frame: track() and redact() joined on the device, a
        redaction.ClipRedaction (frames, track, own, hull_flags).
        frames, boxes, box_smooth, one_euro, fps, chunk_frames: exactly as track takes them; boxes are the F faces of frames[0], at most
        max_batch of them.  mode, blocks, mask, grow, mask_feather, feather: as redact takes them.  smooth=True: with mask='hull' the hull
        is fitted to the tracker's One-Euro points brought back into the frame of each frame's box; False: to the pose head's mu.
        gate: a quality.QualityGate handed to the tracker, or None.
        ONLY THE FACES BOXED ON THE FIRST FRAME ARE FOLLOWED.  A face that enters the clip later is not redacted: detection of new faces
        is out of scope.
        A face the tracker lost on a frame (Track.lost), or that the gate found unsure, keeps the box row the tracker's unchanged state
        gives it; imm_clip_rows hands it NaN landmarks, imm_hull_fit flags it and the paste covers its whole box.  On the first frame
        the tracker scores the faces without losing any, so the gate's verdict is OR-ed into the flags on the device (bit 2 of
        hull_flags): a face the gate finds unsure is covered whole on every frame, the first included.  With mask=None the hull
        launches are not issued and the box is covered anyway.  A lost or unsure face is never shown.
        Per chunk the frames are uploaded and copied into a canvas on the device; per frame the tracker's launches, imm_clip_rows,
        with the mask imm_hull_fit, imm_redact_cells_u8 from the frame's original pixels and imm_redact_u8 run on the detector's stream
        with the box rows the frame before left in device memory.  Between the first and the last frame's launches nothing is copied to
        the host and the stream is not synchronised."""
        from . import redaction as RD
        plan = RD.plan_redact_clip(frames, boxes, self.K, mode, blocks, mask, grow, mask_feather, feather, smooth, box_smooth, one_euro,
                                   fps, chunk_frames, self.max_batch, gate)
        return RD.run_clip(self, plan)

    def annotate(self, photos, boxes=None, landmarks=None, draw=('points', 'box'), size=2.5, thickness=1, labels=None, status=None, grow=1.25,
                 alpha=1.0, return_transform=False, pad=None, label_scale=1):
        """The photos with what the detector found drawn into them: a list of u8 device tensors [h_i, w_i, 3], one per photo, views of
        one packed buffer (what redact returns).  photos, boxes: as redact takes them.  draw: a subset of ('points', 'box', 'hull',
        'label'): the landmarks of every box as the markers of utils/plot_landmarks.py (8 colours x 7 shapes, radius `size` pixels, in
        (0, 32]), the box frame `thickness` pixels wide (an int in [1, 16]) in the colour of the row's status (annotation.STATUS_PALETTE:
        ok, lost, outside, unsure; status: None or int32 [n], imm_track.h's bits with bit 2 for unsure), the outline of the landmark hull
        grown by `grow` (what mask='hull' of morph and redact covers) and labels (None: the row's number; ints in 0..9999) in a 5 x 7
        font of label_scale pixels a dot.  alpha in (0, 1] is the opacity of the markers.  landmarks: f32 [n, K, 2] in the frame of the
        boxes where the caller has them; the pose program is then skipped.  A row whose status has bit 0 set (lost) draws its frame and
        label only.  Rows are applied in row order; a row draws inside its box grown by pad pixels (default ceil(size) + 2), so that a
        marker on the box edge is drawn whole.  include/imm_annotate.h states the rule.
        On the detector's stream, nothing returning to the host: per bucket imm_resize_crop_u8 and the captured pose program (unless
        landmarks is given, or neither points nor hull are drawn), then imm_annotate_points, imm_hull_fit only when the hull is drawn,
        and ONE imm_annotate_u8 launch per call.
        return_transform=True: (photos, an annotation.PhotoAnnotation: rows, points, hull_edges, hull_flags, status)."""
        from . import annotation as AN
        from .generation import PasteSetup
        K = self.K
        plan = AN.plan_annotate(photos, boxes, K, landmarks, draw, size, thickness, labels, status, grow, alpha, 0, pad, label_scale)
        photos, rows, bits = plan.photos, plan.rows, plan.bits
        n, pts, hull = len(rows), bool(bits & AN.BITS['points']), bool(bits & AN.BITS['hull'])
        held = _Held(self.dev)
        lm = None if plan.landmarks is None or not (pts or hull) else held.keep(plan.landmarks.to(device=self.dev, dtype=torch.float32).contiguous())
        buckets = plan_buckets(n, self.max_batch)
        ps = PasteSetup(photos, rows, [(0, n, n)], 0.0, self.dev)                   # all photos, once per call; the links of ONE launch
        held.keep(*ps.tensors())
        extra = {}
        with torch.cuda.device(self.dev):
            palette_d = held.up(plan.palette)
            mu = points = hflags = None
            if pts or hull:
                mu = lm if lm is not None else held.empty(n, K, 2)
                points = held.empty(1, n, K, 2)
            if pts:
                extra.update(marks=points, group_style=held.up(plan.group_style), mark_style=held.up(plan.mark_style))
            if hull:
                grow_d, hflags = held.up(plan.grow), held.empty(n, dtype=torch.int32)
                extra.update(edges=held.empty(n, K, 3))
            if plan.labels is not None:
                extra.update(labels=held.up(plan.labels))
            if plan.status is not None:
                extra.update(status=held.up(plan.status))
        with self._forked(*held):
            if mu is not None:
                if lm is None:
                    for start, count, bucket in buckets:
                        part = slice(start, start + count)
                        self._stage(count, bucket, packed=ps.packed(part))
                        self._run(bucket)
                        mu[part].copy_(self._mu[:count])
                ops.annotate_points(mu, ps.boxes_d, points[0])
            if hull:
                ops.hull_fit(mu, ps.boxes_d, grow_d, extra['edges'], hflags)
            ops.annotate_u8(ps.canvas, ps.offs_d, ps.hw_d, ps.boxes_d, ps.links_d, palette_d, bits, plan.thickness, plan.pad, plan.label_scale,
                            plan.max_pixels, **extra)
        out = unpack_u8(ps.canvas, photos)
        if return_transform:
            return out, AN.PhotoAnnotation(rows, None if points is None else points[0], extra.get('edges'), hflags, plan.status)
        return out

    def annotate_clip(self, frames, boxes=None, track=None, draw=('points', 'box'), trail=0, smooth=True, gate=None, size=2.5, thickness=1,
                      labels=None, grow=1.25, alpha=1.0, pad=None, label_scale=1, box_smooth=0.5, one_euro=OneEuro(), fps=25.0,
                      chunk_frames=32):
        """The faces of a clip followed from its first frame and drawn on every frame: track() and annotate() joined on the device, an
        annotation.ClipAnnotation (frames, track, status).  Exactly one of boxes and track is given.
        boxes: the F faces of frames[0]; frames, box_smooth, one_euro, fps, chunk_frames, gate: exactly as track / redact_clip take them.
        track: a tracking.Track of these frames the caller already has: the tracker is skipped and its points, boxes and flags (and
        qflags) are drawn; the bytes are those of the tracked call that produced it.
        draw, size, thickness, labels, grow, alpha, pad, label_scale: as annotate takes them (labels=None with 'label' numbers the faces).
        trail: an int in [0, 15]: the landmarks of that many earlier frames as fading discs under the markers; the first frames of a clip
        have fewer.  smooth=True draws the tracker's One-Euro points, False its raw points.  The hull is fitted to the frame's own
        landmarks (Track.mu) in the frame's box.
        The frame of a face is coloured by its status, formed on the device: the tracker's flags (bit 0 lost, bit 1 the next box left
        the photo) with the gate's verdict OR-ed in as bit 2; a lost face keeps the box the tracker's unchanged state gives it and draws
        its frame and label only.
        Per chunk the frames are uploaded and copied into a canvas on the device; per frame the tracker's launches, imm_hull_fit when
        the hull is drawn and ONE imm_annotate_u8 launch run on the detector's stream, the marks a view of the tracker's own point
        slots.  Between the first and the last frame's launches nothing is copied to the host and the stream is not synchronised."""
        from . import annotation as AN
        plan = AN.plan_annotate_clip(frames, boxes, track, self.K, draw, trail, smooth, gate, size, thickness, labels, grow, alpha, pad,
                                     label_scale, box_smooth, one_euro, fps, chunk_frames, self.max_batch)
        return AN.run_clip(self, plan)

    def colour_stats(self, photos, boxes=None):
        """The statistics colour matching works from, per box row and channel: (count int64 [n], mean f64 [n, 3], standard deviation f64
        [n, 3]) on the host.  photos, boxes: as morph takes them (a list of u8 arrays; box rows, by default one whole-photo box per
        photo).  The region of a row is the pixels of its box that lie in its photo and in the ellipse inscribed in the box
        (include/imm_colour.h); a row without such a pixel, or with a box of more than 2^30 pixels, has count 0 and NaN.  One
        imm_colour_stats_u8 launch on the caller's stream, the kernel morph(colour > 0) runs; the sums come back as integers and the
        moments are formed on the host in imm_colour_gain's order."""
        from . import morphing as MP
        from .generation import box_areas
        needs = 'photos: %s' % NEEDS_U8
        photos, rows = photos_and_rows(photos, boxes, needs, needs, limit=(65535, 'colour_stats serves at most 65535 rows a call, got %d'))
        with torch.cuda.device(self.dev):
            src, offs_d, hw_d, boxes_d = pack_u8(photos, self.dev, rows)
            sums = torch.empty(len(rows), 7, dtype=torch.int64, device=self.dev)
            ops.colour_stats_u8(src, offs_d, hw_d, boxes_d, int(box_areas(rows).max()), sums)
            return MP.colour_moments(sums.cpu().numpy())

    def unalign(self, photos, aligned, alignment, feather=0.125):
        """align() run backwards: the photos with every row's aligned face pasted back where align() took it from: a list of u8 device
        tensors [h_i, w_i, 3], one per photo, views of one packed buffer (as ImageGenerator.repose returns them).
        photos: the list of u8 arrays align() was given.  aligned: f32 [n, So, So, >= 3] on the host or the device (channels 0..2 are
        read; a device tensor with dense pixels of one stride is read in place), So == alignment.out_size: the aligned faces, edited
        or generated in the canonical frame.  alignment: what align(photos, ..., return_transform=True) returned (similarity or
        affine; the tps map is not inverted: NotImplementedError).  feather in [0, 0.5]: the share of the aligned frame's side over
        which the paste fades into the photo (0: a hard paste).
        The photos are packed once; imm_unalign_maps inverts the rows' maps on the device (the coefficients never come back to the
        host) and imm_unalign_u8 pastes the rows in row order (a later row blends over an earlier paste), sampling each face
        bilinearly, without a pre-filter: a face much smaller in the photo than So x So is point-sampled."""
        from . import alignment as AL
        from .generation import compose_links
        photos, rows, n, So, feather = plan_unalign(photos, getattr(aligned, 'shape', np.shape(aligned)), alignment, feather)
        faces = torch.as_tensor(aligned)
        if faces.dtype != torch.float32:
            faces = faces.float()
        with torch.cuda.device(self.dev):                 # everything on the caller's stream: the detector's programs are not run
            faces = faces.to(self.dev) if faces.is_cuda else ops.to_device_pinned(faces, self.dev)
            ld = faces.stride(2)
            if faces.stride(3) != 1 or ld < 3 or faces.stride(1) != So * ld or faces.stride(0) != So * So * ld:
                faces = faces.contiguous()
            coef, geom = (ops.to_device_pinned(torch.as_tensor(a), self.dev, torch.float32).contiguous()
                          for a in (alignment.coef, alignment.geom))
            canvas, offs_d, hw_d, boxes_d = pack_u8(photos, self.dev, rows)              # all photos, once per call
            fwd = torch.empty(n, 6, device=self.dev)
            bbox = torch.empty(n, 4, dtype=torch.int32, device=self.dev)
            ops.unalign_maps(coef, geom, boxes_d, hw_d, self.S, So, fwd, bbox)
            inv_ramp = AL.unalign_inv_ramp(feather, So)
            for start in range(0, n, UNALIGN_MAX_ROWS):
                part = slice(start, min(start + UNALIGN_MAX_ROWS, n))
                links_d = ops.to_device_pinned(compose_links(rows[part]), self.dev)
                ops.unalign_u8(canvas, offs_d, hw_d, boxes_d[part], links_d, fwd[part], bbox[part], inv_ramp, faces[part],
                               unalign_grid_pixels(photos, rows[part]))
        return unpack_u8(canvas, photos)
