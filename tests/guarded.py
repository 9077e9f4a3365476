"""Poisoned buffers and guard bands: the harness of tests/test_gpu_guarded.py (a plain helper
module: no plugin, no fixture, no pytest setting).

The property it lets a test state: *a result is a function of its inputs only, and a kernel
touches only its own bytes*.

* :func:`guarded_allocations` serves ``torch.empty`` / ``zeros`` / ``empty_like`` / ``zeros_like``
  / ``Tensor.new_empty`` / ``Tensor.new_zeros`` from allocations whose every byte is ``fill``: the
  body sits ``GUARD`` bytes in, keeps the 512-byte alignment of the caching allocator (so the
  vector paths taken are the production ones) and is zeroed only for the ``zeros`` family.
  Whatever the code under test leaves unwritten stays poison; whatever it writes outside the body
  lands in a guard band that :meth:`Arena.check` reads back.
* :func:`rehome` copies an *input* tensor into such a home of its own, so the kernels see it alone
  between two guards instead of next to the neighbouring column of a packed buffer;
  :func:`rehome_batch`, :func:`rehome_blocks` and :func:`rehome_model` do that for every device
  tensor of an ``ActionBatch``, a ``FeatureBlocks`` and a ``TreeEnsemble``.  Their handle's
  ``check()`` also asserts that the bodies still hold the bytes put in: kernels do not write
  their inputs.

Two fills: ``0xFF`` reads as NaN in f64 / f32, -1 in every signed integer, 255 in bytes;
``0x5A`` as a huge finite float (about 1.8e127 in f64, 1.5e16 in f32), a large positive int64, 90
in bytes.  A stray
value enters a sum, a comparison and an index differently in the two cases, and a result that is
a function of its inputs only is the same bytes under both.

``GUARD`` is twice the largest row tile in bytes (the bool tile quantum of 1024 rows x 8 B per f64
row -> 16 KiB), from the tile constants of ``socceraction_amd._native``, rounded to 512.

The patches go on ``torch`` itself (several functions ``import torch`` locally, a per-module proxy
would miss them) and only for the duration of the ``with`` body.  Requests for another device type
than the guarded one (default ``'cuda'``; the CPU tests of the harness pass ``'cpu'`` to run the
very same wrapper on host memory), pinned requests and requests with other keywords
(``memory_format``, ``out``, a non-contiguous ``_like`` source ...) pass through to the original;
an ``empty`` one is then filled with ``fill`` and has no guard.
"""
from __future__ import annotations

import contextlib
import os
import sys
from typing import Callable, Dict, List, Optional, Tuple

import torch

from socceraction_amd import _native

FILLS = (0xFF, 0x5A)
_ALIGN = 512


def _round(n: int, a: int) -> int:
    return (n + a - 1) // a * a


GUARD = _round(2 * max(_native.SA_BOOL_TILE_QUANTUM, _native.SA_NUM_TILE_QUANTUM) * 8, _ALIGN)
assert GUARD >= 16384 and GUARD % _ALIGN == 0

_HERE = os.path.abspath(__file__)
_PATCHED_TORCH = ('empty', 'zeros', 'empty_like', 'zeros_like')
_PATCHED_TENSOR = ('new_empty', 'new_zeros')
_full = torch.full  # never patched: what the harness itself allocates with


def _call_site() -> str:
    """file:line (function) of the nearest frame outside this module."""
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    if f is None:  # pragma: no cover
        return '?'
    return f'{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} ({f.f_code.co_name})'


class _Alloc:
    __slots__ = ('backing', 'nbytes', 'shape', 'dtype', 'site', 'pristine')

    def __init__(self, backing, nbytes, shape, dtype, site):
        self.backing, self.nbytes, self.shape, self.dtype, self.site = backing, nbytes, shape, dtype, site
        self.pristine = None  # rehomed inputs: the bytes put in

    def name(self) -> str:
        return f'{tuple(self.shape)} {self.dtype} allocated at {self.site}'


class Arena:
    """Guarded allocations of one fill: keeps every backing buffer alive, counts them, and reads
    the guards (and the bodies of rehomed inputs) back in :meth:`check`."""

    def __init__(self, fill: int, device_type: str = 'cuda', fill_stream=None):
        if not 0 <= int(fill) <= 255:
            raise ValueError('fill is one byte')
        self.fill = int(fill)
        self.device_type = device_type
        # None: the fill is ordered on the requester's current stream, like the allocation's first
        # use.  A stream: the fill runs there and is waited for before the body is handed out, so
        # the poison is in memory whatever the requester's stream is waiting for
        # (tests/test_gpu_streams.py builds under a stalled stream).
        self.fill_stream = fill_stream
        self.allocs: List[_Alloc] = []
        self.count = 0          # guarded allocations
        self.passed_through = 0  # requests handed to the original (no guard)

    # ------------------------------------------------------------------ allocation
    def alloc(self, shape, dtype: torch.dtype, device, zero: bool, site: Optional[str] = None) -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * _itemsize(dtype)
        with self._filling():
            backing = _full((GUARD + nbytes + GUARD,), self.fill, dtype=torch.uint8, device=device)
            body = backing[GUARD:GUARD + nbytes]
            if zero:
                body.zero_()
        self.allocs.append(_Alloc(backing, nbytes, shape, dtype, site or _call_site()))
        self.count += 1
        return body.view(dtype).view(shape)

    @contextlib.contextmanager
    def _filling(self):
        """The stream the fill runs on; with a ``fill_stream``, waited for on the way out."""
        if self.fill_stream is None:
            yield
            return
        with torch.cuda.stream(self.fill_stream):
            yield
        self.fill_stream.synchronize()

    def rehome(self, t: torch.Tensor, site: Optional[str] = None) -> torch.Tensor:
        """A guarded copy of ``t`` (made contiguous); its bytes are checked by :meth:`check`."""
        src = t.detach().contiguous()
        out = self.alloc(src.shape, src.dtype, src.device, zero=False, site=site or _call_site())
        out.copy_(src)
        a = self.allocs[-1]
        a.pristine = a.backing[GUARD:GUARD + a.nbytes].clone()
        return out

    # ------------------------------------------------------------------ checks
    def check(self) -> None:
        """Every guard byte is still ``fill`` and every rehomed body holds what was put in; the
        first offender is named by shape, dtype and call site.  One host read for all of them."""
        if not self.allocs:
            return
        by_dev: Dict[torch.device, list] = {}
        for i, a in enumerate(self.allocs):  # (allocation, weight, 0-dim bool) per region
            b = a.backing
            flags = by_dev.setdefault(b.device, [])
            flags.append((i, 4, (b[:GUARD] != self.fill).any()))
            flags.append((i, 2, (b[GUARD + a.nbytes:] != self.fill).any()))
            if a.pristine is not None and a.nbytes:
                flags.append((i, 1, (b[GUARD:GUARD + a.nbytes] != a.pristine).any()))
        hit: Dict[int, int] = {}
        for flags in by_dev.values():
            for (i, wgt, _), v in zip(flags, torch.stack([f for _, _, f in flags]).tolist()):
                if v:
                    hit[i] = hit.get(i, 0) + wgt
        bad = list(hit.items())
        if not bad:
            return
        lines = []
        for i, v in sorted(bad):
            a = self.allocs[i]
            what = []
            if v >= 4:
                what.append(f'{self._first(a, front=True)} in front of the body')
            if v & 2:
                what.append(f'{self._first(a, front=False)} behind the body')
            if v & 1:
                what.append('input body modified')
            lines.append(f'{a.name()}: ' + ', '.join(what))
        raise AssertionError(f'guard bytes (fill 0x{self.fill:02X}) or input bodies changed:\n  '
                             + '\n  '.join(lines))

    def _first(self, a: _Alloc, front: bool) -> str:
        g = a.backing[:GUARD] if front else a.backing[GUARD + a.nbytes:]
        hit = (g != self.fill).nonzero().reshape(-1)
        n = int(hit.numel())
        d = GUARD - int(hit[-1]) if front else int(hit[0]) + 1
        return f'{n} stray byte(s), nearest {d} byte(s)'


_ITEMSIZE: Dict[torch.dtype, int] = {}


def _itemsize(dtype: torch.dtype) -> int:
    if dtype not in _ITEMSIZE:
        _ITEMSIZE[dtype] = torch.tensor([], dtype=dtype).element_size()
    return _ITEMSIZE[dtype]


# ---------------------------------------------------------------------- the patches
def _size_of(args) -> Optional[Tuple[int, ...]]:
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    try:
        return tuple(int(s) for s in args)
    except (TypeError, ValueError):
        return None


def _device_of(dev) -> torch.device:
    return torch.tensor(0).device if dev is None else torch.device(dev)  # None: the default device


def _fill_passed(t, fill: int, zero: bool):
    """An unguarded ``empty``: poisoned all the same."""
    if not zero and isinstance(t, torch.Tensor) and t.numel() and t.layout == torch.strided:
        # the whole fresh storage, whatever the strides
        torch.tensor([], dtype=torch.uint8, device=t.device).set_(t.untyped_storage()).fill_(fill)
    return t


def _make(arena: Arena, orig: Callable, zero: bool, like: bool, method: bool) -> Callable:
    def wrapper(*args, **kw):
        site = _call_site()
        plain = set(kw) <= {'dtype', 'device', 'size'}
        src = None
        if like or method:
            src, rest = (args[0], args[1:]) if args else (None, ())
            plain = plain and isinstance(src, torch.Tensor) and src.layout == torch.strided
            if like:
                plain = plain and not rest and 'size' not in kw and src.is_contiguous()
                size = tuple(src.shape) if plain else None
            else:
                size = _size_of((kw['size'],)) if 'size' in kw else _size_of(rest)
        else:
            size = _size_of((kw['size'],)) if 'size' in kw else _size_of(args)
        if plain and size is not None and all(s >= 0 for s in size):
            dtype = kw.get('dtype') or (src.dtype if src is not None else torch.get_default_dtype())
            dev = torch.device(kw['device']) if kw.get('device') is not None else \
                (src.device if src is not None else _device_of(None))
            if dev.type == arena.device_type and isinstance(dtype, torch.dtype):
                return arena.alloc(size, dtype, dev, zero, site)
        arena.passed_through += 1
        t = orig(*args, **kw)
        with arena._filling():
            return _fill_passed(t, arena.fill, zero)
    wrapper.__wrapped__ = orig
    return wrapper


@contextlib.contextmanager
def guarded_allocations(fill: int, device_type: str = 'cuda', fill_stream=None):
    """Serve the ``empty`` / ``zeros`` family from guarded, ``fill``-poisoned allocations for the
    duration of the body (see the module docstring); yields the :class:`Arena`.  The originals
    are back when the body ends, also when it raises, and the guards are checked on a normal
    exit.  ``fill_stream``: see :class:`Arena`."""
    arena = Arena(fill, device_type, fill_stream)
    saved = []
    try:
        for name in _PATCHED_TORCH:
            orig = getattr(torch, name)
            assert not hasattr(orig, '__wrapped__'), 'guarded_allocations does not nest'
            saved.append((torch, name, True, orig))
            setattr(torch, name, _make(arena, orig, zero='zeros' in name, like='like' in name, method=False))
        for name in _PATCHED_TENSOR:
            own = name in vars(torch.Tensor)
            orig = getattr(torch.Tensor, name)
            saved.append((torch.Tensor, name, own, orig))
            setattr(torch.Tensor, name, _make(arena, orig, zero='zeros' in name, like=False, method=True))
        yield arena
    finally:
        for obj, name, own, orig in reversed(saved):
            if own:
                setattr(obj, name, orig)
            else:  # inherited from the C base class: drop the override
                delattr(obj, name)
    arena.check()


# ---------------------------------------------------------------------- rehomed inputs
def rehome(t: torch.Tensor, fill: int, arena: Optional[Arena] = None) -> torch.Tensor:
    """``t`` copied into a guarded home of its own (``arena``: collect it there)."""
    arena = arena or Arena(fill, t.device.type)
    return arena.rehome(t, _call_site())


def rehome_batch(ab, fill: int) -> Arena:
    """Every column of an ``ActionBatch`` (``seg_of_block`` included) alone between two guards,
    in place: ``struct()`` reads ``data_ptr()`` at call time.  Returns the handle to ``check()``."""
    arena = Arena(fill, ab.device.type)
    ab._seg_blocks()
    for k in list(ab.cols):
        ab.cols[k] = arena.rehome(ab.cols[k], f'ActionBatch.cols[{k!r}]')
    return arena


def rehome_blocks(fb, fill: int) -> Arena:
    """The f64 / i64 / bool / bitmap blocks of a ``FeatureBlocks``, in place."""
    arena = Arena(fill, fb.device.type)
    for name in ('bool_block', 'f64_block', 'i64_block', 'bool_bits'):
        t = getattr(fb, name)
        if t is not None:
            setattr(fb, name, arena.rehome(t, f'FeatureBlocks.{name}'))
    return arena


def rehome_model(ens, dev, fill: int) -> Arena:
    """The device tensors of ``TreeEnsemble._device(dev)``, in place: the node, root and depth
    tables and the staged-walk tables cached there by earlier ``predict_blocks`` calls (call it
    after the first prediction of each kind, which builds them)."""
    arena = Arena(fill, torch.device(dev).type)

    def walk(rec: dict, path: str) -> None:
        for k, t in list(rec.items()):
            if isinstance(t, torch.Tensor):
                rec[k] = arena.rehome(t, f'{path}[{k!r}]')
            elif isinstance(t, dict):
                walk(t, f'{path}[{k if isinstance(k, str) else k[0]!r}]')
    walk(ens._device(dev), 'TreeEnsemble._device()')
    return arena
