"""A side stream behind a stalled default stream: the harness of tests/test_gpu_streams.py (a
plain helper module like tests/guarded.py: no plugin, no fixture, no pytest setting).

The property it lets a test state: *a call uses the stream it is given and nothing else; a cached
table is usable from any stream once its builder has returned*.

* :func:`stall` enqueues a bounded spin (``torch.cuda._sleep``) on a stream and returns an event
  recorded behind it.  The spin is timed, never released by the host: a wrong dependency on the
  stalled stream shows as a completed event and a failed assertion, not as a hang.  One stall is
  at most ``STALL_CAP_MS``.
* :class:`StreamRun` has the interface of ``test_gpu_guarded.Run`` (``call``, ``home``, ``batch``,
  ``own``, ``keep``, ``keep_frame``, ``finish``), so the ``case(run)`` closures of
  tests/test_gpu_guarded.py drive it as they stand; :func:`both_passes` runs a case twice.

  *Default pass.*  The case runs on the default stream; ``keep`` records result bytes and ``call``
  records each call's wall time ``t_k`` (host time plus a synchronise of the stream).  As in the
  side pass each call runs once untimed first: the first use of a torch op in a process costs
  hundreds of ms (the first ``column_exps`` of a fresh process took 417 ms, of a warm one 0.6 ms),
  which says nothing about how long the stalled run will take.

  *Side pass.*  The k-th ``call`` makes the side stream wait for what the case body queued on the
  default stream (the caller orders the inputs), runs ``fn`` once on the side stream (allocator
  misses, a fresh scratch slot and first-use pinned allocations do not land in the timed run),
  then stalls the default stream for ``d_k = max(floor, 4 * t_k)``, runs ``fn`` under
  ``torch.cuda.stream(side)``, synchronises the side stream and asserts at once that the stall's
  event has NOT completed: no part of the call ran on, or waited for, the default stream, and
  nothing synchronised the device.  What the case body does outside ``call`` (its ``.cpu()``, its
  oracle assertions) queues behind the stall on the default stream as usual.  ``finish`` returns
  the kept bytes; :func:`both_passes` compares the two passes and names the first differing byte.

  A stall that is over when checked FAILS the case (no skip, no retry); the message gives
  ``t_k``, ``d_k`` and the side call's time, which tells "too slow" from "waited on the default
  stream".  A call of more than ``CALL_MAX_MS`` on the default stream fails too: four times it
  would not fit under the cap.
  ``device_wide`` is the allow-list: a call it names needs the whole device for a reason it
  states, runs behind a stall of at most ``DEVICE_WIDE_STALL_MS`` and must outlast it (an entry
  that does not wait is stale and fails); its oracle assertions and the byte comparison hold as
  for every other call.

  A limit of the side pass: the first, unstalled run of ``fn`` frees its results to the side
  stream's allocator pool, and the stalled run most likely gets those very blocks back.  If one
  kernel of the stalled run went to stream 0, a consumer on the side stream would find the first
  run's correct bytes there, and the case body's own read on the default stream comes behind the
  stray kernel and is correct too.  So a misrouted kernel that only OVERWRITES its output with
  the same values escapes the side pass; one that zeroes or accumulates (a memset, an atomic
  sum, a counter) gives wrong bytes and is caught, as is anything that makes the call wait.
* :func:`control` -- once per process: a stalled default stream, ``torch.ones(4096).sum()`` on a
  side stream, the side stream synchronised, the stall still pending.  The runtime serves all
  streams of a process from a few hardware queues (``GPU_MAX_HW_QUEUES``, 4 here) and two
  streams that share one run in order, whatever the library does: of the 32 streams
  ``torch.cuda.Stream()`` hands out in turn, 7 queued behind the default stream where this was
  measured.  So the control runs on every pool stream (:func:`pool`), the side passes use the
  first independent one (:func:`side_stream`), and :func:`steer_pool` sees to it that a stream a
  call makes for itself is an independent one too.  If NO pool stream is independent, torch's
  side streams are not independent of the default stream on this runtime; the control fails with
  that message and nothing else is asserted.  ``floor`` is ten times the control's time: the
  slowest of ``CONTROL_RUNS`` runs of the whole control on the chosen stream (stall enqueued, op,
  synchronise, query).

Measured on an MI355X (printed by tests/test_gpu_streams.py under ``-s``; ``MEASURED`` below):
2,398,304 spin cycles per ms; the control 0.043 ms, so ``floor`` = 0.435 ms; 7 of the 32 pool
streams queue behind the default stream; the largest ``t_k`` of a family 170.7 ms (the first
``column_exps`` of the process, first-use costs included), of a warm call 30.5 ms
(``compute_batch``).
"""
from __future__ import annotations

import contextlib
import gc
import time
from typing import Dict, List, Optional

import numpy as np
import torch

STALL_CAP_MS = 1000.0   # no single spin longer than this
STALL_FACTOR = 4.0      # d_k = max(floor, STALL_FACTOR * t_k)
FLOOR_FACTOR = 10.0     # floor = FLOOR_FACTOR * the control's time
CALL_MAX_MS = 250.0     # a call of a chosen case on the default stream
CONTROL_RUNS = 5
FILL = 0xFF             # what ``run.fill`` reads as for the cases that rehome inputs themselves

# For the record (one MI355X, tests/test_gpu_streams.py alone in its process); the tests use
# what they measure in their own process.  ``pool``: the 32 pool streams in hand-out order, x =
# queues behind the default stream.  ``t_max_ms``: the largest t_k per family, first-use costs of
# the default pass included.
MEASURED = {'cycles_per_ms': 2398304, 'control_ms': 0.043, 'floor_ms': 0.435,
            'pool': '......x...x...x...x...x...x...x.',
            't_max_ms': {'chained': 170.69, 'convert / dribbles': 22.09, 'group sums': 0.40, 'learner': 2.51,
                         'logistic moments': 0.60, 'metrics': 0.22, 'pandas boundary': 30.47, 'public path': 6.79,
                         'select': 9.19, 'top-k': 108.43, 'trees': 0.35, 'vaep': 53.38, 'xT large grid': 0.53,
                         'xT small grids': 1.15}}

_STATE: Dict[str, object] = {}


# ---------------------------------------------------------------------- pure helpers (CPU-tested)
def cycles_per_ms_from(c1: int, t1: float, c2: int, t2: float) -> float:
    """Spin cycles per millisecond from two spins of ``c1 < c2`` cycles that took ``t1`` and
    ``t2`` ms: the difference cancels the launch and event cost common to both."""
    if not (c2 > c1 > 0 and t2 > t1 > 0):
        raise ValueError(f'calibration spins out of order: {c1} cycles {t1} ms, {c2} cycles {t2} ms')
    return (c2 - c1) / (t2 - t1)


def stall_length(t_k: float, floor: float) -> float:
    """``d_k`` in ms for a call that took ``t_k`` ms on the default stream."""
    if t_k > CALL_MAX_MS:
        raise AssertionError(f'a call of {t_k:.1f} ms on the default stream: over {CALL_MAX_MS:.0f} ms, '
                             f'{STALL_FACTOR:.0f} times it does not fit under the {STALL_CAP_MS:.0f} ms cap')
    d = max(float(floor), STALL_FACTOR * float(t_k))
    if d > STALL_CAP_MS:
        raise AssertionError(f'a stall of {d:.1f} ms is over the {STALL_CAP_MS:.0f} ms cap (floor {floor:.1f} ms)')
    return d


def same_bytes(a: dict, b: dict, family: str, what: str = 'differs between the default and the side stream') -> None:
    """The kept results of two passes (``name -> (dtype, shape, bytes or device uint8 tensor)``)
    are the same names in the same order and the same bytes; the first differing byte is named."""
    assert list(a) == list(b) and a, (family, list(a), list(b))
    for k in a:
        assert a[k][:2] == b[k][:2], (family, k, a[k][:2], b[k][:2])
        x, y = a[k][2], b[k][2]
        if isinstance(x, torch.Tensor):
            if torch.equal(x, y):
                continue
            x, y = x.cpu().numpy(), y.cpu().numpy()
        elif x != y:
            x, y = np.frombuffer(x, np.uint8), np.frombuffer(y, np.uint8)
        else:
            continue
        at = int(np.flatnonzero(x != y)[0])
        raise AssertionError(f'{family}: {k} {a[k][0]} {a[k][1]} {what}: '
                             f'{int((x != y).sum())} bytes differ, the first at byte {at}')


# ---------------------------------------------------------------------- stalls
def calibration() -> float:
    """Spin cycles per millisecond of ``torch.cuda._sleep`` on the current device, measured once
    per process from two short spins timed with events."""
    if 'cpm' not in _STATE:
        st = torch.cuda.current_stream()

        def timed(cycles: int) -> float:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            torch.cuda._sleep(cycles)
            b.record(st)
            b.synchronize()
            return a.elapsed_time(b)

        timed(1000)  # loads the spin kernel
        c1, c2 = 250_000, 1_000_000
        _STATE['cpm'] = cycles_per_ms_from(c1, timed(c1), c2, timed(c2))
    return _STATE['cpm']


def stall(stream, ms: float):
    """A spin of ``ms`` milliseconds enqueued on ``stream``; returns an event recorded behind it."""
    if not 0 < ms <= STALL_CAP_MS:
        raise ValueError(f'a stall is between 0 and {STALL_CAP_MS:.0f} ms, not {ms}')
    cycles = int(ms * calibration())
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        ev.record(stream)
    return ev


PROBE_MS = 3.0          # the stall of one independence probe
POOL_MAX = 64           # torch hands out 32 pool streams per priority; twice that ends the search
DEVICE_WIDE_STALL_MS = 10.0  # the longest stall in front of an allow-listed call


def _probe_op():
    return torch.ones(4096, device='cuda').sum()


def independent(blocker, s) -> tuple:
    """``(pending, ms)``: ``blocker`` stalled for ``PROBE_MS``, ``torch.ones(4096).sum()`` on ``s``
    and a synchronise of ``s``; ``pending`` says the stall was not over then, i.e. ``s`` does not
    queue behind ``blocker``; ``ms`` is the time of all that, from enqueueing the stall to the
    query."""
    t0 = time.perf_counter()
    ev = stall(blocker, PROBE_MS)
    with torch.cuda.stream(s):
        v = _probe_op()
    s.synchronize()
    pending = not ev.query()
    ms = (time.perf_counter() - t0) * 1e3
    blocker.synchronize()
    assert float(v) == 4096.0
    return pending, ms


def pool() -> tuple:
    """``(streams, handles, good)`` of torch's stream pool in the order ``torch.cuda.Stream()``
    hands it out (round robin), once per process; ``good[i]``: stream i is independent of the
    default stream.  The runtime serves all streams of a process from a few hardware queues
    (``GPU_MAX_HW_QUEUES``), bound at a stream's first use, and streams that share one run in
    order: on a four-queue runtime about every fourth pool stream queues behind the default
    stream.  That is the runtime's, not the library's, so the harness looks before it asserts."""
    if 'pool' not in _STATE:
        calibration()
        default = torch.cuda.default_stream()
        streams = [torch.cuda.Stream()]
        while len(streams) <= POOL_MAX:
            s = torch.cuda.Stream()
            if s.cuda_stream == streams[0].cuda_stream:
                break
            streams.append(s)
        else:
            raise AssertionError(f'torch.cuda.Stream() did not come round after {POOL_MAX} streams')
        good = []
        for s in streams:
            with torch.cuda.stream(s):  # first use: binds the stream's hardware queue
                _probe_op()
            s.synchronize()
            good.append(independent(default, s)[0])
        _STATE['pool'] = (streams, [s.cuda_stream for s in streams], good)
    return _STATE['pool']


def control() -> float:
    """The control (see the module docstring), once per process; returns ``floor`` in ms.  A
    failed control is remembered and raised again: the module that asked asserts nothing else."""
    if 'floor' in _STATE:
        return _STATE['floor']
    if 'control_error' in _STATE:
        raise AssertionError(_STATE['control_error'])
    streams, _, good = pool()
    if not any(good):
        _STATE['control_error'] = (
            f'control: on each of the {len(streams)} streams torch hands out, torch.ones(4096).sum() returned '
            f'only after a {PROBE_MS:.0f} ms stall of the default stream was over: side streams are not '
            'independent of the default stream on this runtime, and no case of this module means anything')
        raise AssertionError(_STATE['control_error'])
    side = streams[good.index(True)]
    worst = 0.0
    for _ in range(CONTROL_RUNS):
        pending, ms = independent(torch.cuda.default_stream(), side)
        worst = max(worst, ms)
        if not pending:
            _STATE['control_error'] = (
                f'control: torch.ones(4096).sum() on a side stream took {ms:.2f} ms and a {PROBE_MS:.0f} ms stall '
                'of the default stream was over when it returned, on a stream that was independent of it a '
                'moment ago: no case of this module means anything')
            raise AssertionError(_STATE['control_error'])
    _STATE['side'] = side
    _STATE['control_ms'] = worst
    _STATE['floor'] = FLOOR_FACTOR * worst
    return _STATE['floor']


def side_stream():
    """The side stream of every side pass: the first pool stream independent of the default one."""
    control()
    return _STATE['side']


def second_stream(first):
    """A pool stream independent of the default stream and of ``first``."""
    control()
    streams, handles, good = pool()
    for s, g in zip(streams, good):
        if g and s.cuda_stream != first.cuda_stream and independent(first, s)[0]:
            return s
    raise AssertionError('no pool stream is independent of both the default stream and the first side stream')


def steer_pool(k: int = 2) -> None:
    """Draw pool streams until the next ``k`` that ``torch.cuda.Stream()`` hands out are
    independent of the default stream: a stream the call under test makes for itself (the copy
    stream of ``pipeline.value_frames``) then does not queue behind the stall by the runtime's
    doing."""
    streams, handles, good = pool()
    n = len(streams)
    for _ in range(2 * n):
        i = handles.index(torch.cuda.Stream().cuda_stream)
        if all(good[(i + 1 + j) % n] for j in range(k)):
            return
    raise AssertionError(f'no {k} consecutive pool streams are independent of the default stream: '
                         + ''.join('.' if g else 'x' for g in good))


def measured() -> dict:
    """What this process measured: cycles per ms, the control's time, the floor."""
    good = _STATE['pool'][2] if 'pool' in _STATE else []
    return {'cycles_per_ms': _STATE.get('cpm'), 'control_ms': _STATE.get('control_ms'),
            'floor_ms': _STATE.get('floor'), 'pool': ''.join('.' if g else 'x' for g in good)}


# ---------------------------------------------------------------------- the runner
T_MAX: Dict[str, float] = {}  # family -> the largest t_k of the cases that ran (ms)
COLLECT_MS: List[tuple] = []  # (family, ms of the full collection in front of its two passes)


@contextlib.contextmanager
def _no_gc():
    """The timed part of a call in either pass: a collection of the host's garbage is no part of
    the call.  :func:`both_passes` collects before it starts and records how long that took
    (``COLLECT_MS``): 310 - 380 ms per full collection late in the whole suite's process (3 ms with
    this module alone), more than the 250 ms a call may take."""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


class StreamRun:
    """One pass of a case: ``times=None`` is the default pass (which measures them), a list of
    the default pass's ``t_k`` the side pass."""

    def __init__(self, family: str, times: Optional[List[float]] = None, once=(), device_wide=None):
        self.family, self.fill = family, FILL
        self.side_pass = times is not None
        self.times: List[float] = [] if times is None else times
        self.once = tuple(once)  # qualified names of calls that cannot be run twice
        # the allow-list: ``device_wide(what, args, kw)`` gives the reason a call needs the whole
        # device, or None; such a call runs behind a short stall and must outlast it
        self.device_wide = device_wide
        self.k = 0
        self.handles, self.out = [], {}
        self.side = side_stream() if self.side_pass else None
        # (what, t_k, d_k, side call's time, pending, allow-listed) of the side pass's calls
        self.stalls: List[tuple] = []

    # ------------------------------------------------------------------ calls
    def call(self, fn, *args, **kw):
        what = getattr(fn, '__qualname__', repr(fn))
        if not self.side_pass:
            st = torch.cuda.current_stream()
            if what not in self.once:  # first use in this process (a cold torch op costs 100s of ms)
                fn(*args, **kw)
                st.synchronize()
            with _no_gc():
                t0 = time.perf_counter()
                res = fn(*args, **kw)
                st.synchronize()
                t = (time.perf_counter() - t0) * 1e3
            self.times.append(t)
            T_MAX[self.family] = max(T_MAX.get(self.family, 0.0), t)
            return res
        assert self.k < len(self.times), f'{self.family}: the side pass makes more calls than the default pass'
        t_k = self.times[self.k]
        self.k += 1
        d_k = stall_length(t_k, control())
        allowed = self.device_wide(what, args, kw) if self.device_wide is not None else None
        if allowed:
            d_k = min(d_k, DEVICE_WIDE_STALL_MS)
        default, side = torch.cuda.default_stream(), self.side
        side.wait_stream(default)  # the caller orders the inputs
        if what not in self.once:
            with torch.cuda.stream(side):  # first use on this stream
                fn(*args, **kw)
            # a result that sits in a reference cycle keeps its device blocks until the collector
            # runs; the young generation holds it, and collecting that is cheap
            gc.collect(0)
        side.synchronize()
        steer_pool()
        with _no_gc():
            ev = stall(default, d_k)
            t0 = time.perf_counter()
            with torch.cuda.stream(side):
                res = fn(*args, **kw)
            side.synchronize()
            pending = not ev.query()
            t_side = (time.perf_counter() - t0) * 1e3
        self.stalls.append((what, t_k, d_k, t_side, pending, bool(allowed)))
        if allowed:
            assert not pending, (
                f'{self.family}: call {self.k - 1} ({what}) is on the allow-list ({allowed}) but returned in '
                f'{t_side:.3f} ms with a {d_k:.3f} ms stall of the default stream still pending: it does not need '
                'the whole device here; take it off the list')
            return res
        assert pending, (
            f'{self.family}: call {self.k - 1} ({what}): the stall of the default stream was already over when the '
            f'call returned on the side stream: t_k = {t_k:.3f} ms on the default stream, d_k = {d_k:.3f} ms, the '
            f'side call took {t_side:.3f} ms (a call that waited for the default stream or the device returns '
            'just after d_k, one that is too slow well after it)')
        return res

    # ------------------------------------------------------------------ inputs
    def own(self, handle):
        self.handles.append(handle)
        return handle

    def home(self, a):
        """A host array or device tensor as a device input: uploaded on the current stream (the
        default one outside ``call``) and synchronised there."""
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        out = t.cuda().clone() if t.is_cuda else t.cuda()
        torch.cuda.current_stream().synchronize()
        return out

    def batch(self, B, d, atomic=False, flip=True):
        ab = B.ActionBatch.from_columns({c: np.array(v) for c, v in d.items()}, atomic=atomic, flip=flip)
        torch.cuda.current_stream().synchronize()
        return ab

    # ------------------------------------------------------------------ results
    def keep(self, name, t):
        if isinstance(t, torch.Tensor) and t.numel() * t.element_size() > 1 << 24:  # compared on the device
            t = t.detach().contiguous().clone()
            self.out[name] = (str(t.dtype), tuple(t.shape), t.view(-1).view(torch.uint8))
            return
        if isinstance(t, torch.Tensor):
            t = t.detach().contiguous().cpu().numpy()
        self.out[name] = (str(np.asarray(t).dtype), np.asarray(t).shape, np.ascontiguousarray(t).tobytes())

    def keep_frame(self, name, df):
        for c in df.columns:
            v = df[c].to_numpy()
            self.keep(f'{name} {c}', v.astype(str) if v.dtype == object else v)
        self.keep(f'{name} index', np.asarray(df.index))

    def finish(self):
        if self.side_pass:
            assert self.k == len(self.times), f'{self.family}: the side pass made {self.k} of {len(self.times)} calls'
        for h in self.handles:  # rehomed inputs: guards intact, bodies unchanged
            h.check()
        torch.cuda.synchronize()
        return self.out


def both_passes(family: str, case, once=(), device_wide=None) -> StreamRun:
    """``case(run)`` on the default stream, then on a side stream behind a stalled default stream;
    the kept results are the same bytes.  Returns the side pass (its ``stalls`` for the record)."""
    control()
    t0 = time.perf_counter()
    gc.collect()
    COLLECT_MS.append((family, (time.perf_counter() - t0) * 1e3))
    first = StreamRun(family, None, once, device_wide)
    case(first)
    a = first.finish()
    second = StreamRun(family, first.times, once, device_wide)
    case(second)
    b = second.finish()
    same_bytes(a, b, family)
    return second
