"""One comparison and guarded buffers for the per-kernel parity tests.

close()         |got - ref| <= atol_frac * max|ref| + rtol * |ref| for EVERY element: a NaN or an inf in `got` fails (the earlier
                helpers tested `err > tol`, which a NaN never satisfies, so an unwritten NaN-filled element counted as good).
out() / inp()   an output / operand as a contiguous view into guard band | body | guard band.  Every byte of the bands (and of an
                output's body) starts as 0xFF — a NaN in f32, bf16 and f16 — so a store past either end of the tensor lands in a
                band and is found by check_guards(), a load past either end that reaches arithmetic turns the result NaN and is
                found by close(), and an element the kernel never writes stays NaN instead of holding a previous case's result.
check_guards()  every band of every buffer made since the last call, compared as bytes on the buffer's own device.
untouched()     every byte of a view is still 0xFF: for padding the kernel's contract leaves to the caller.

Nothing here needs a GPU at import time; every allocator takes the device, so the helpers themselves are tested on the CPU
(tests/test_guarded_cpu.py).
"""
import math
import os
import sys

import torch

ALIGN = 256                      # the body keeps the alignment the kernels' 16-byte vector accesses rely on (torch's allocator: 512)
MIN_GUARD = 64 * 1024
_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}

_live = []                       # [what, region (uint8, guard + body + guard), guard bytes, body bytes]


def close(got, ref, rtol, atol_frac, what):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ref_ok = torch.isfinite(ref)
    assert bool(ref_ok.all()), '%s: the REFERENCE holds %d non-finite of %d elements: a bug of the test, not of the kernel' % (
        what, int((~ref_ok).sum()), ref.numel())
    scale = float(ref.abs().max()) + 1e-30
    err = (got - ref).abs()
    tol = atol_frac * scale + rtol * ref.abs()
    bad = ~(err <= tol)          # NOT err > tol: a NaN compares false both ways, and must count as bad
    if bool(bad.any()):
        finite = err[torch.isfinite(err)]
        raise AssertionError(
            '%s: %d/%d elements off (%d NaN, %d inf in got), max err %.4g (ref max %.4g), first bad idx %s got %.6g ref %.6g' % (
                what, int(bad.sum()), bad.numel(), int(torch.isnan(got).sum()), int(torch.isinf(got).sum()),
                float(finite.max()) if finite.numel() else float('nan'), scale,
                tuple(int(i) for i in bad.nonzero()[0]), float(got[bad][0]), float(ref[bad][0])))


def _caller(depth):
    f = sys._getframe(depth + 1)
    return '%s:%d' % (os.path.basename(f.f_code.co_filename), f.f_lineno)


def guard_bytes(shape, dtype):
    """max(64 KiB, one item along dim 0) rounded up to 256 bytes: an overrun by a whole image still lands inside the band."""
    item = math.prod(shape[1:]) * torch.empty(0, dtype=dtype).element_size()
    return -(-max(MIN_GUARD, item) // ALIGN) * ALIGN


def _alloc(shape, dtype, device, what):
    shape = tuple(int(s) for s in shape)
    body = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
    g = guard_bytes(shape, dtype)
    parent = torch.full((g + body + g + ALIGN,), 0xFF, dtype=torch.uint8, device=device)
    off = -parent.data_ptr() % ALIGN
    region = parent[off:off + g + body + g]
    view = region[g:g + body].view(dtype).view(shape)
    _live.append(['%s %s%s' % (what, str(dtype).replace('torch.', ''), list(shape)), region, g, body])
    return view


def out(shape, dtype, device, fill=None, what=None):
    """A kernel output: NaN body (all-ones bytes) between two 0xFF guard bands.  `fill` (a number or a tensor of that shape) is for
    a buffer the kernel accumulates into or that must start from given values: it keeps those contents and still gets the bands."""
    view = _alloc(shape, dtype, device, what or _caller(1))
    if isinstance(fill, torch.Tensor):
        view.copy_(fill)
    elif fill is not None:
        view.fill_(fill)
    return view


def inp(tensor, device, what=None, depth=1):
    """A kernel operand: `tensor` copied into a guarded body on `device`; a read outside it meets 0xFF bytes (NaN in every float type)."""
    view = _alloc(tensor.shape, tensor.dtype, device, what or _caller(depth))
    view.copy_(tensor)
    return view


def live():
    return len(_live)


def reset():
    """Forget every registered buffer without checking it (start of a test: what an earlier, failed test left behind)."""
    del _live[:]


def check_guards():
    """Every band of every registered buffer must still be all 0xFF.  One small reduction per band on its device, one transfer
    for all of them; the registry is cleared whatever the outcome."""
    bufs = list(_live)
    del _live[:]
    if not bufs:
        return
    counts = []
    for _what, region, g, body in bufs:
        counts.append((region[:g] != 0xFF).sum() + (region[g + body:] != 0xFF).sum())
    counts = torch.stack([c.to(counts[0].device) for c in counts]).cpu().tolist()
    hit = [b for b, c in zip(bufs, counts) if c]
    if not hit:
        return
    lines = []
    for what, region, g, body in hit:
        for band, lo, n in (('before', 0, g), ('after', g + body, g)):
            diff = (region[lo:lo + n] != 0xFF).nonzero().flatten()
            if diff.numel():
                first = int(diff[0])
                where = 'byte %d before the first element' % (g - first) if band == 'before' else 'byte %d past the last element' % first
                lines.append('%s: guard band %s the body touched: %d byte(s) differ, first at band offset %d (%s)' % (
                    what, band, diff.numel(), first, where))
    raise AssertionError('write outside a tensor: ' + '; '.join(lines))


def untouched(view):
    """True if every byte of `view` (any strides) is still 0xFF, i.e. nothing wrote it since out() made the buffer."""
    if view.numel() == 0:
        return True
    bits = view.contiguous().view(_INT_OF_SIZE[view.element_size()])
    return bool((bits == (0xFF if view.element_size() == 1 else -1)).all())
