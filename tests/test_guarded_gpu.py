"""tests/guarded.py on the MI355X: the device-side byte comparison of check_guards() and untouched().  The planted writes are
host-issued copies into the guarded allocation itself; no kernel of the library runs here."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded                                                              # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(autouse=True)
def _gpu_and_empty_registry():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    guarded.check_guards()
    yield
    guarded.reset()


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16, torch.float16], ids=['f32', 'bf16', 'f16'])
def test_planted_writes_on_the_device_are_reported(dt):
    for index_of, band in ((lambda y: -1, 'before'), (lambda y: y.numel(), 'after')):
        clean = guarded.out((2, 128, 128, 32), dt, DEV, what='clean')       # one item = 1 MiB (f32): bands wider than 64 KiB
        y = guarded.out((3, 5, 8), dt, DEV, what='victim')
        assert y.is_cuda and y.is_contiguous() and y.data_ptr() % 256 == 0 and bool(torch.isnan(y).all()) and guarded.untouched(y)
        y.fill_(0.5); clean.fill_(0.5)
        assert not guarded.untouched(y)
        _what, region, g, _body = guarded._live[-1]
        region.view(dt)[g // y.element_size() + index_of(y)] = 1.0
        with pytest.raises(AssertionError) as e:
            guarded.check_guards()
        msg = str(e.value)
        es = y.element_size()
        assert 'victim' in msg and 'clean' not in msg and 'guard band %s the body' % band in msg, msg
        assert '%d byte(s) differ, first at band offset %d ' % (es, g - es if band == 'before' else 0) in msg, msg
        assert guarded.live() == 0


def test_clean_device_buffers_pass_and_inp_copies():
    src = torch.arange(3 * 7 * 10.).reshape(3, 7, 10).to(torch.bfloat16)
    x = guarded.inp(src, DEV)
    y = guarded.out((3, 7, 16), torch.bfloat16, DEV)
    y[..., :10] = x * 2
    assert torch.equal(x.cpu(), src) and guarded.untouched(y[..., 10:]) and not guarded.untouched(y[..., 9:])
    guarded.check_guards()
