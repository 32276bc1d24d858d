"""The photo-ingest kernel tests (tests/test_ingest_gpu.py), validated without a GPU: for every exact case the index-built expectation
equals the oracle bit for bit (oracle/tps_oracle.warp, tests/alignment_reference.warp) and holds the stated shares of padding and
image; the tight photo buffer is what its name says; and the wrappers refuse every malformed call before anything is launched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alignment_reference as R                                             # noqa: E402
import guarded                                                              # noqa: E402
import ingest_data as D                                                     # noqa: E402
from oracle import tps_oracle as T                                          # noqa: E402


@pytest.mark.parametrize('shape', D.TPS_EXACT, ids=D.TPS_EXACT_IDS)
def test_tps_exact_expectation_is_the_oracle(shape):
    B, H, W, C, hc, wc = shape
    img, w, expect, inside = D.tps_exact_case(*shape)
    np.testing.assert_array_equal(T.warp(img, w, hc, wc), expect)
    assert img.min() >= 1 and np.array_equal(expect == 0, np.broadcast_to(~inside[..., None], expect.shape))
    # at least 5 % of the output pixels are the padding (exact zeros), at least 50 % come from the image
    assert 1.0 - inside.mean() >= 0.05 and inside.mean() >= 0.50, inside.mean()
    assert (H * W) % 256 != 0 and B % 8 != 0
    # every sample its own transform, every channel its own pattern
    assert len({w[b].tobytes() for b in range(B) if b % 4 != 3}) == B - B // 4
    assert all(not np.array_equal(img[..., a], img[..., b]) for a in range(C) for b in range(a))


def test_tps_exact_shapes_cover_the_tile_tails_and_both_orientations():
    assert sorted(s[0] % 8 for s in D.TPS_EXACT) == [1, 2, 3, 3, 4, 5]
    assert any(s[1] > s[2] for s in D.TPS_EXACT) and any(s[1] < s[2] for s in D.TPS_EXACT)
    assert {s[3] for s in D.TPS_EXACT} == {1, 2, 3, 4, 5, 8}


@pytest.mark.parametrize('So', D.ALIGN_SO)
def test_align_exact_expectation_is_the_reference(So):
    owner, geom, coef, rows, cols = D.align_exact_maps(So)
    t = R.jittered_grid_template(D.ALIGN_K, 6)
    assert len(owner) % 8 == 3 and (So * So) % 256 != 0 or So >= 16
    for images, own in ((D.align_photos(), owner), (list(D.align_f32_sources()), np.arange(len(owner)))):
        expect, inside = D.align_expect(images, own, rows, cols)
        for c in (coef, D.as_tps_coef(coef)):                    # the same maps as m3 = 3 and as a tps set with zero radial rows
            np.testing.assert_array_equal(R.warp(images, own, geom, c, t, D.S, So), expect)
        assert np.array_equal(expect == 0, np.broadcast_to(~inside[..., None], expect.shape))
        # at least 10 % of the pixels are outside the photo, at least 30 % inside
        assert 1.0 - inside.mean() >= 0.10 and inside.mean() >= 0.30, inside.mean()
    assert not np.array_equal(D.align_f32_sources(), np.rint(D.align_f32_sources()))


def test_pack_tight_is_tight():
    ims = D.align_photos()
    buf, offs, hw = D.pack_tight(ims)
    assert ims[-1].shape[:2] == (31, 47) and all(o % 2 == 1 for o in offs)
    assert buf.size == 1 + sum(im.size for im in ims) and offs[-1] + ims[-1].size == buf.size
    for im, o, (h, w) in zip(ims, offs, hw):
        assert np.array_equal(buf[o:o + im.size].reshape(h, w, 3), im)
    assert buf[0] == 0xFF and int(buf[1:].max()) <= 63
    with pytest.raises(AssertionError):
        D.pack_tight([np.full((2, 2, 3), 64, np.uint8)])
    pbuf, poffs, _ = D.pack_padded(ims)
    assert all(o % 16 == 0 for o in poffs) and pbuf.size % 16 == 0


def test_flush_resize_ends_on_the_last_source_pixel():
    """The kernel's own coordinate formula, (out - 1) * f32((in - 1) / (out - 1)), at the last output row and column."""
    for size in D.FLUSH_SIZES:
        for n_in, n_out in zip(size, D.FLUSH_RESIZE):
            scale = np.float32(n_in - 1) / np.float32(n_out - 1)
            assert float(scale) in (2.0, 3.0, 4.0) and float(np.float32(n_out - 1) * scale) == n_in - 1


def test_wrappers_refuse_malformed_calls_before_any_launch():
    """On CPU tensors: a refusal that came after the launch would have handed the library host pointers."""
    from imm_amd import ops
    guarded.reset()
    calls = D.refused_calls(ops, 'cpu')
    assert len({name for name, _ in calls}) == len(calls)
    for name, call in calls:
        with pytest.raises(ValueError):
            call()
            pytest.fail('%s: accepted' % name)
    guarded.check_guards()
