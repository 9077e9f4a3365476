"""The host-side parts of tests/streams.py (no GPU): the stall length, the calibration arithmetic
and the byte comparison of two passes."""
import numpy as np
import pytest

import streams as ss

torch = pytest.importorskip('torch')


def test_stall_length_is_the_floor_or_four_times_the_call():
    assert ss.stall_length(0.1, 2.0) == 2.0
    assert ss.stall_length(0.5, 2.0) == 2.0
    assert ss.stall_length(3.0, 2.0) == 12.0
    assert ss.stall_length(ss.CALL_MAX_MS, 2.0) == ss.STALL_CAP_MS == ss.STALL_FACTOR * ss.CALL_MAX_MS


def test_a_call_over_the_limit_or_a_floor_over_the_cap_fails():
    with pytest.raises(AssertionError, match='over 250 ms'):
        ss.stall_length(ss.CALL_MAX_MS + 0.001, 2.0)
    with pytest.raises(AssertionError, match='over the 1000 ms cap'):
        ss.stall_length(1.0, ss.STALL_CAP_MS + 1)


def test_stall_refuses_a_spin_over_the_cap_before_it_touches_a_device():
    for ms in (0, -1.0, ss.STALL_CAP_MS + 0.001):
        with pytest.raises(ValueError):
            ss.stall(None, ms)


def test_calibration_is_the_slope_of_two_spins():
    # 100 cycles per microsecond and 0.02 ms of launch cost in both spins
    assert ss.cycles_per_ms_from(250_000, 2.52, 1_000_000, 10.02) == pytest.approx(100_000)
    for bad in ((1_000_000, 10.0, 250_000, 2.5), (250_000, 2.5, 1_000_000, 2.5), (0, 1.0, 10, 2.0)):
        with pytest.raises(ValueError):
            ss.cycles_per_ms_from(*bad)


def _kept(**arrays):
    return {k: (str(v.dtype), v.shape, v.tobytes()) for k, v in arrays.items()}


def test_same_bytes_names_the_first_differing_byte():
    a = np.arange(6, dtype=np.float64)
    b = a.copy()
    ss.same_bytes(_kept(x=a, y=a[:3]), _kept(x=b, y=b[:3]), 'family')
    b[2] = np.nextafter(2.0, 3.0)  # one ulp: the lowest byte of element 2
    with pytest.raises(AssertionError, match=r'family: x float64 \(6,\) .*1 bytes differ, the first at byte 16'):
        ss.same_bytes(_kept(x=a), _kept(x=b), 'family')
    with pytest.raises(AssertionError):  # other names, another order, nothing kept
        ss.same_bytes(_kept(x=a), _kept(y=a), 'family')
    with pytest.raises(AssertionError):
        ss.same_bytes(_kept(x=a, y=a), _kept(y=a, x=a), 'family')
    with pytest.raises(AssertionError):
        ss.same_bytes({}, {}, 'family')
    with pytest.raises(AssertionError):  # the same bytes under another dtype
        ss.same_bytes(_kept(x=a), _kept(x=a.view(np.int64)), 'family')


def test_same_bytes_compares_device_style_entries_as_tensors():
    t = torch.arange(16, dtype=torch.uint8)
    u = t.clone()
    ss.same_bytes({'x': ('torch.uint8', (16,), t)}, {'x': ('torch.uint8', (16,), u)}, 'family')
    u[5] = 99
    with pytest.raises(AssertionError, match='the first at byte 5'):
        ss.same_bytes({'x': ('torch.uint8', (16,), t)}, {'x': ('torch.uint8', (16,), u)}, 'family')


def test_the_default_pass_times_calls_and_keeps_bytes_without_a_device():
    """``keep`` / ``keep_frame`` / ``finish`` bookkeeping of a default pass on host values."""
    import pandas as pd
    run = ss.StreamRun.__new__(ss.StreamRun)
    run.family, run.side_pass, run.out, run.handles, run.k, run.times = 'family', False, {}, [], 0, []
    run.keep('a', np.arange(3, dtype=np.int32))
    run.keep('t', torch.arange(4, dtype=torch.float32))
    run.keep_frame('f', pd.DataFrame({'c': [1.5, 2.5], 's': ['u', 'v']}, index=[7, 9]))
    assert list(run.out) == ['a', 't', 'f c', 'f s', 'f index']
    assert run.out['a'] == ('int32', (3,), np.arange(3, dtype=np.int32).tobytes())
    assert run.out['t'][:2] == ('float32', (4,)) and run.out['f index'][2] == np.array([7, 9]).tobytes()
