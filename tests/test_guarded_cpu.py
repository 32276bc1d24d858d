"""tests/guarded.py on the CPU: the comparison every kernel parity test goes through must reject what the earlier one let pass (NaN
anywhere, an all-NaN result), and the guard bands must report a write on either side of a tensor.  The planted writes are host-issued
and land inside the test's own allocation."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded                                                              # noqa: E402

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']


@pytest.fixture(autouse=True)
def _empty_registry():
    guarded.check_guards()
    yield
    guarded.reset()


def _ref():
    return torch.tensor([[1.0, -2.0, 4.0], [0.5, 0.0, -3.0]])


# ----------------------------------------------------------------------------------------------------------------------------
# close
# ----------------------------------------------------------------------------------------------------------------------------
def test_close_accepts_equal_and_just_inside_tolerance():
    ref = _ref()
    guarded.close(ref.clone(), ref, 1e-2, 1e-3, 'equal')
    got = ref.clone()
    got[0, 0] = 1.0 + 0.0139              # tol = 1e-3 * 4 + 1e-2 * 1 = 0.014
    got[1, 1] = -0.0039                   # tol = 1e-3 * 4 = 0.004 at a zero reference
    guarded.close(got, ref, 1e-2, 1e-3, 'inside')


def test_close_rejects_just_outside_tolerance():
    ref = _ref()
    got = ref.clone()
    got[0, 0] = 1.0 + 0.0141
    with pytest.raises(AssertionError) as e:
        guarded.close(got, ref, 1e-2, 1e-3, 'outside')
    msg = str(e.value)
    assert msg.startswith('outside: 1/6 elements off (0 NaN, 0 inf in got)') and 'first bad idx (0, 0)' in msg, msg


def test_close_rejects_one_nan():
    ref = _ref()
    got = ref.clone()
    got[1, 2] = float('nan')
    with pytest.raises(AssertionError) as e:
        guarded.close(got, ref, 1e-2, 1e-3, 'one nan')
    msg = str(e.value)
    assert '1/6 elements off (1 NaN, 0 inf in got)' in msg and 'first bad idx (1, 2)' in msg, msg


@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
def test_close_rejects_all_nan(dt):
    ref = _ref()
    got = torch.full(ref.shape, float('nan'), dtype=dt)
    with pytest.raises(AssertionError) as e:
        guarded.close(got, ref, 1e-2, 1e-3, 'all nan')
    assert '6/6 elements off (6 NaN, 0 inf in got)' in str(e.value), str(e.value)


@pytest.mark.parametrize('v', [float('inf'), float('-inf')], ids=['plus_inf', 'minus_inf'])
def test_close_rejects_inf(v):
    ref = _ref()
    got = ref.clone()
    got[0, 1] = v
    with pytest.raises(AssertionError) as e:
        guarded.close(got, ref, 1e-2, 1e-3, 'inf')
    assert '1/6 elements off (0 NaN, 1 inf in got)' in str(e.value), str(e.value)


def test_close_rejects_shape_mismatch():
    ref = _ref()
    with pytest.raises(AssertionError):
        guarded.close(ref.reshape(3, 2), ref, 1e-2, 1e-3, 'shape')
    with pytest.raises(AssertionError):
        guarded.close(ref[:, :2], ref, 1e-2, 1e-3, 'shape')


@pytest.mark.parametrize('v', [float('nan'), float('inf')], ids=['nan', 'inf'])
def test_close_rejects_non_finite_reference_as_a_bug_of_the_test(v):
    ref = _ref()
    ref[0, 2] = v
    with pytest.raises(AssertionError) as e:
        guarded.close(ref.clone(), ref, 1e-2, 1e-3, 'bad ref')       # even a `got` with the very same bits
    assert 'REFERENCE' in str(e.value) and 'bug of the test' in str(e.value), str(e.value)


def test_close_message_keeps_its_count_fields():
    ref = _ref()
    got = ref.clone()
    got[0, 0] = float('nan'); got[0, 1] = float('inf'); got[1, 0] = 0.75
    with pytest.raises(AssertionError) as e:
        guarded.close(got, ref, 1e-2, 1e-3, 'fields')
    m = re.match(r'fields: (\d+)/(\d+) elements off \((\d+) NaN, (\d+) inf in got\), max err ([0-9.e+-]+) \(ref max ([0-9.e+-]+)\), '
                 r'first bad idx \((\d+), (\d+)\) got (\S+) ref (\S+)$', str(e.value))
    assert m is not None, str(e.value)
    assert [int(m.group(i)) for i in (1, 2, 3, 4)] == [3, 6, 1, 1]
    assert float(m.group(5)) == 0.25 and float(m.group(6)) == 4.0           # the largest FINITE error, not NaN
    assert (m.group(7), m.group(8), m.group(9), float(m.group(10))) == ('0', '0', 'nan', 1.0)


# ----------------------------------------------------------------------------------------------------------------------------
# out / inp / check_guards / untouched
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', [(3, 5, 7, 10), (7,), (2, 200, 200, 8)], ids=['odd', 'seven', 'item_above_64k'])
def test_out_shape_dtype_alignment_and_nan_body(shape, dt):
    y = guarded.out(shape, dt, 'cpu')
    assert tuple(y.shape) == shape and y.dtype == dt and y.is_contiguous() and y.device.type == 'cpu'
    assert y.data_ptr() % 256 == 0
    assert bool(torch.isnan(y).all()) and guarded.untouched(y)
    item = y[0].numel() * y.element_size()
    g = guarded.guard_bytes(shape, dt)
    assert g % 256 == 0 and g >= max(64 * 1024, item) and g < max(64 * 1024, item) + 256
    _what, region, gb, body = guarded._live[-1]
    assert gb == g and body == y.numel() * y.element_size() and region.numel() == 2 * g + body
    assert region.data_ptr() + g == y.data_ptr() and bool((region == 0xFF).all())
    guarded.check_guards()
    assert guarded.live() == 0


def test_out_with_fill_and_inp_keep_their_contents_between_bands():
    a = guarded.out((4, 6), torch.float32, 'cpu', fill=0)
    b = guarded.out((4, 6), torch.int32, 'cpu', fill=7)
    src = torch.arange(24.).reshape(4, 6).to(torch.bfloat16)
    c = guarded.out((4, 6), torch.bfloat16, 'cpu', fill=src)
    d = guarded.inp(src.t(), 'cpu')                                          # a non-contiguous source
    assert float(a.abs().max()) == 0.0 and bool((b == 7).all()) and torch.equal(c, src)
    assert torch.equal(d, src.t()) and d.is_contiguous() and d.data_ptr() % 256 == 0
    for _what, region, g, body in guarded._live:
        assert bool((region[:g] == 0xFF).all()) and bool((region[g + body:] == 0xFF).all())
    assert guarded.live() == 4
    guarded.check_guards()


def _plant(y, index):
    """One element written at `index` elements from the start of y's body (negative: before it), through a view of the same
    allocation: the write stays inside the buffer guarded.out() made."""
    _what, region, g, _body = guarded._live[-1]
    region.view(y.dtype)[g // y.element_size() + index] = 1.0


@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
def test_planted_write_before_the_body_is_reported(dt):
    y = guarded.out((3, 5, 8), dt, 'cpu', what='victim')
    y.fill_(0.5)
    _plant(y, -1)
    with pytest.raises(AssertionError) as e:
        guarded.check_guards()
    msg = str(e.value)
    assert 'victim' in msg and 'guard band before the body' in msg and 'after the body' not in msg, msg
    es, g = y.element_size(), guarded.guard_bytes(y.shape, dt)
    # 1.0 is 0x3F800000 / 0x3F80 / 0x3C00: no byte of it is 0xFF
    assert '%d byte(s) differ, first at band offset %d (byte %d before the first element)' % (es, g - es, es) in msg, msg
    assert guarded.live() == 0                                              # cleared even on failure
    guarded.check_guards()


@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
def test_planted_write_after_the_body_is_reported(dt):
    guarded.out((9,), torch.float32, 'cpu', what='bystander')
    y = guarded.out((3, 5, 8), dt, 'cpu', what='victim')
    y.fill_(0.5)
    _plant(y, y.numel())
    with pytest.raises(AssertionError) as e:
        guarded.check_guards()
    msg = str(e.value)
    assert 'victim' in msg and 'bystander' not in msg and 'guard band after the body' in msg and 'before the body' not in msg, msg
    assert re.search(r'first at band offset [0-3] \(byte [0-3] past the last element\)', msg), msg
    assert guarded.live() == 0


def test_body_writes_and_clean_buffers_pass():
    y = guarded.out((5, 7), torch.float16, 'cpu')
    x = guarded.inp(torch.ones(3, 3), 'cpu')
    y.fill_(3.0)                                                             # first to last element: not a guard's business
    x.mul_(2.0)
    guarded.check_guards()
    guarded.check_guards()                                                   # empty registry


def test_default_name_is_the_calling_line():
    guarded.out((2, 2), torch.float32, 'cpu')
    assert re.match(r'test_guarded_cpu\.py:\d+ float32\[2, 2\]$', guarded._live[-1][0]), guarded._live[-1][0]


@pytest.mark.parametrize('dt', DTYPES, ids=IDS)
def test_untouched_tells_a_written_element_from_an_unwritten_one(dt):
    y = guarded.out((2, 4, 4, 16), dt, 'cpu')
    assert guarded.untouched(y) and guarded.untouched(y[..., 10:]) and guarded.untouched(y[..., :0])
    y[..., :10] = 0.25
    assert guarded.untouched(y[..., 10:]) and not guarded.untouched(y[..., 9:]) and not guarded.untouched(y)
    y[1, 3, 3, 15] = 0.0                                                     # one element, the last one
    assert not guarded.untouched(y[..., 10:]) and guarded.untouched(y[0, ..., 10:])
    # a NaN the kernel computed is not the fill pattern: float('nan') is 0x7FC00000 / 0x7FC0 / 0x7E00, not all ones
    z = guarded.out((4,), dt, 'cpu')
    z[2] = float('nan')
    assert not guarded.untouched(z) and guarded.untouched(z[:2])
