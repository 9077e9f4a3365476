"""tests/guarded.py on host memory (no GPU): the very wrapper the device tests use, with
``device_type='cpu'`` so that plain host requests are the guarded ones.  Pinned requests and
requests with other keywords still pass through."""
import numpy as np
import pytest

import guarded as gd

torch = pytest.importorskip('torch')

DTYPES = (torch.bool, torch.uint8, torch.int16, torch.int32, torch.int64, torch.float32, torch.float64)
SHAPES = ((3, 5), (7,), (2, 3, 4), (0,), (0, 5), ())


def _backing_of(arena, i=-1):
    return arena.allocs[i].backing


def _fill_value(dtype, fill):
    """What a body of ``fill`` bytes reads as in ``dtype`` (as raw bytes of one element)."""
    return np.full(torch.tensor([], dtype=dtype).element_size(), fill, np.uint8)


def _forms(shape, dtype):
    """(name, zero, call) of every patched form for one request."""
    like = torch.ones(shape, dtype=torch.float32).to(dtype)
    other = torch.ones(2, dtype=torch.float32)
    return [
        ('empty', False, lambda: torch.empty(shape, dtype=dtype, device='cpu')),
        ('zeros', True, lambda: torch.zeros(shape, dtype=dtype, device='cpu')),
        ('empty_like', False, lambda: torch.empty_like(like)),
        ('zeros_like', True, lambda: torch.zeros_like(like)),
        ('new_empty', False, lambda: other.new_empty(shape, dtype=dtype)),
        ('new_zeros', True, lambda: other.new_zeros(shape, dtype=dtype)),
    ]


def test_guard_width_comes_from_the_tile_constants():
    from socceraction_amd import _native
    assert gd.GUARD == 2 * max(_native.SA_BOOL_TILE_QUANTUM, _native.SA_NUM_TILE_QUANTUM) * 8
    assert gd.GUARD >= 16384 and gd.GUARD % 512 == 0
    assert gd.FILLS == (0xFF, 0x5A)


@pytest.mark.parametrize('fill', gd.FILLS)
@pytest.mark.parametrize('dtype', DTYPES, ids=str)
def test_every_form_shape_and_dtype(dtype, fill):
    """Shape, dtype, contiguity, alignment and contents of every patched form: the body starts
    GUARD bytes (a multiple of 512) into a backing buffer that is ``fill`` everywhere else; it is
    ``fill`` for the empty family and zero for the zeros family; zero-size requests work."""
    for shape in SHAPES:
        for name, zero, call in _forms(shape, dtype):
            with gd.guarded_allocations(fill, device_type='cpu') as arena:
                t = call()
                assert arena.count == 1 and arena.passed_through == 0, (name, shape)
                b = _backing_of(arena)
            tag = (name, shape, dtype)
            assert t.shape == torch.Size(shape) and t.dtype == dtype, tag
            assert t.is_contiguous() and t.device.type == 'cpu', tag
            nbytes = t.numel() * t.element_size()
            assert b.dtype == torch.uint8 and b.numel() == 2 * gd.GUARD + nbytes, tag
            if t.numel():  # an empty tensor reports no address
                assert t.data_ptr() - b.data_ptr() == gd.GUARD and gd.GUARD % 512 == 0, tag
                assert t.data_ptr() % t.element_size() == 0, tag
            raw = b.numpy()
            assert (raw[:gd.GUARD] == fill).all() and (raw[gd.GUARD + nbytes:] == fill).all(), tag
            assert (raw[gd.GUARD:gd.GUARD + nbytes] == (0 if zero else fill)).all(), tag
            if zero:
                assert not t.to(torch.float64).any(), tag
            elif t.numel() and dtype != torch.bool:
                got = t.reshape(-1)[:1].numpy().view(np.uint8)
                assert (got == _fill_value(dtype, fill)).all(), tag
            arena.check()


def test_fills_read_as_documented():
    with gd.guarded_allocations(0xFF, device_type='cpu'):
        f = torch.empty(4, dtype=torch.float64, device='cpu')
        g = torch.empty(4, dtype=torch.float32, device='cpu')
        i = torch.empty(4, dtype=torch.int32, device='cpu')
        u = torch.empty(4, dtype=torch.uint8, device='cpu')
    assert f.isnan().all() and g.isnan().all() and (i == -1).all() and (u == 255).all()
    with gd.guarded_allocations(0x5A, device_type='cpu'):
        f = torch.empty(4, dtype=torch.float64, device='cpu')
        g = torch.empty(4, dtype=torch.float32, device='cpu')
        i = torch.empty(4, dtype=torch.int64, device='cpu')
        u = torch.empty(4, dtype=torch.uint8, device='cpu')
    assert f.isfinite().all() and (f > 1e127).all() and (f < 1e128).all()
    assert g.isfinite().all() and (g > 1e16).all()
    assert (i == 0x5A5A5A5A5A5A5A5A).all() and (u == 90).all()


def test_size_spellings_and_default_dtype():
    with gd.guarded_allocations(0x5A, device_type='cpu') as arena:
        a = torch.empty(3, 5, device='cpu')
        b = torch.zeros([3, 5])
        c = torch.empty(torch.Size((3, 5)), dtype=torch.int16)
        d = torch.zeros(size=(3, 5), dtype=torch.int16)
        assert arena.count == 4 and arena.passed_through == 0
    for t in (a, b, c, d):
        assert t.shape == (3, 5)
    assert a.dtype == b.dtype == torch.get_default_dtype() and c.dtype == d.dtype == torch.int16


def test_other_devices_and_keywords_pass_through():
    """A request for another device type than the guarded one, a pinned one and one with other
    keywords go to the original: no guard, an ``empty`` one poisoned all the same."""
    with gd.guarded_allocations(0x5A) as arena:  # guards 'cuda': host requests pass through
        h = torch.empty(6, dtype=torch.int32)
        z = torch.zeros(6, dtype=torch.int32)
        assert arena.count == 0 and arena.passed_through == 2
    assert (h == 0x5A5A5A5A).all() and not z.any()
    with gd.guarded_allocations(0xFF, device_type='cpu') as arena:
        src = torch.ones(4, 6).t()
        assert not src.is_contiguous()
        s = torch.empty_like(src)                                  # strides follow the source
        m = torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)
        o = torch.empty(3, out=torch.ones(3))
        r = torch.zeros(3, requires_grad=True)
        assert arena.count == 0 and arena.passed_through == 4
    assert s.shape == (6, 4) and m.shape == (2, 3, 4, 5) and m.is_contiguous(memory_format=torch.channels_last)
    assert m.isnan().all() and o.shape == (3,) and r.requires_grad and not r.detach().any()


def test_pinned_request_passes_through():
    with gd.guarded_allocations(0x5A, device_type='cpu') as arena:
        try:
            p = torch.empty(8, dtype=torch.uint8, pin_memory=True)
            z = torch.zeros(8, dtype=torch.uint8, pin_memory=True)
        except RuntimeError:  # no accelerator runtime to pin with: the request still reached the original
            p = z = None
        assert arena.count == 0 and arena.passed_through >= 1
    if p is not None:
        assert (p == 0x5A).all() and not z.any()


@pytest.mark.parametrize('where', ['before', 'after'])
@pytest.mark.parametrize('fill', gd.FILLS)
def test_stray_write_next_to_a_body_is_reported(fill, where):
    """One byte in front of and one byte behind a body: check() names the allocation by shape,
    dtype and call site; the other allocations are not blamed; the exit check raises too."""
    def reported(msg):
        assert '(3, 5) torch.float64' in msg and 'test_guarded_host.py' in msg
        assert 'test_stray_write_next_to_a_body_is_reported' in msg
        assert ('in front of' if where == 'before' else 'behind') in msg and 'nearest 1 byte' in msg
        assert ('behind' if where == 'before' else 'in front of') not in msg
        assert 'torch.int32' not in msg and 'torch.bool' not in msg and 'input body' not in msg

    # the explicit check, inside a body that ends clean (the stray byte is put back)
    with gd.guarded_allocations(fill, device_type='cpu') as arena:
        torch.empty(9, dtype=torch.int32, device='cpu')
        t = torch.zeros((3, 5), dtype=torch.float64, device='cpu')
        torch.empty(2, dtype=torch.bool, device='cpu')
        arena.check()
        at = gd.GUARD - 1 if where == 'before' else gd.GUARD + t.numel() * 8
        _backing_of(arena, 1)[at] = fill ^ 1
        with pytest.raises(AssertionError) as inner:
            arena.check()
        _backing_of(arena, 1)[at] = fill
    reported(str(inner.value))
    # the check on exit: the block holds nothing but the allocations and the stray write
    with pytest.raises(AssertionError) as ei:
        with gd.guarded_allocations(fill, device_type='cpu') as arena:
            torch.empty(9, dtype=torch.int32, device='cpu')
            t = torch.zeros((3, 5), dtype=torch.float64, device='cpu')
            torch.empty(2, dtype=torch.bool, device='cpu')
            _backing_of(arena, 1)[gd.GUARD - 1 if where == 'before' else gd.GUARD + t.numel() * 8] = fill ^ 1
    assert ei.type is AssertionError and str(ei.value).startswith('guard bytes')
    reported(str(ei.value))
    assert not hasattr(torch.empty, '__wrapped__')


def test_rehomed_input_is_a_guarded_copy_and_writes_to_it_are_reported():
    src = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    arena = gd.Arena(0xFF, 'cpu')
    t = gd.rehome(src, 0xFF, arena)
    assert t.data_ptr() != src.data_ptr() and torch.equal(t, src) and t.is_contiguous()
    assert t.data_ptr() - _backing_of(arena).data_ptr() == gd.GUARD
    v = gd.rehome(src.t(), 0xFF, arena)  # a non-contiguous source arrives contiguous
    assert v.is_contiguous() and torch.equal(v, src.t())
    arena.check()
    t[1, 2] = -1.0
    with pytest.raises(AssertionError, match='input body modified') as ei:
        arena.check()
    assert '(3, 4) torch.float64' in str(ei.value) and '(4, 3)' not in str(ei.value)
    t[1, 2] = src[1, 2]
    arena.check()
    _backing_of(arena, 1)[gd.GUARD + 12 * 8] = 0
    with pytest.raises(AssertionError, match='behind the body'):
        arena.check()


def test_rehome_helpers_replace_every_tensor():
    class _Batch:
        device = torch.device('cpu')

        def __init__(self):
            self.cols = {'c0': torch.rand(5, dtype=torch.float64), 'team': torch.arange(5, dtype=torch.int32),
                         'seg_of_block': torch.zeros(1, dtype=torch.int32)}

        def _seg_blocks(self):
            return None

    ab = _Batch()
    before = {k: v.clone() for k, v in ab.cols.items()}
    h = gd.rehome_batch(ab, 0x5A)
    assert h.count == 3
    for k, v in ab.cols.items():
        assert torch.equal(v, before[k]) and v.data_ptr() != before[k].data_ptr()
    h.check()
    ab.cols['team'][0] = 9
    with pytest.raises(AssertionError, match="cols\\['team'\\]"):
        h.check()

    class _Blocks:
        device = torch.device('cpu')
        bool_block = None
        f64_block = torch.rand(1, 2, 16, dtype=torch.float64)
        i64_block = torch.zeros(1, 1, 16, dtype=torch.int64)
        bool_bits = torch.ones(3, 1, dtype=torch.int64)

    fb = _Blocks()
    h = gd.rehome_blocks(fb, 0xFF)
    assert h.count == 3 and fb.bool_block is None and torch.equal(fb.f64_block, _Blocks.f64_block)
    h.check()

    class _Model:
        _dev = {'dev': 'cpu', 'nodes': torch.arange(8, dtype=torch.uint8), 'depth': None,
                ('staged', b'k'): {'leaf': torch.rand(4), 'n_num': 2, 'roots': None}, ('x', b''): False}

        def _device(self, dev):
            return self._dev

    m = _Model()
    h = gd.rehome_model(m, 'cpu', 0xFF)
    assert h.count == 2 and m._dev['nodes'].tolist() == list(range(8))
    assert m._dev[('staged', b'k')]['n_num'] == 2
    h.check()


def test_originals_are_back_after_exit_and_after_an_exception():
    names = ('empty', 'zeros', 'empty_like', 'zeros_like')
    before = {n: getattr(torch, n) for n in names}
    own = {n: n in vars(torch.Tensor) for n in ('new_empty', 'new_zeros')}
    meth = {n: getattr(torch.Tensor, n) for n in own}
    with gd.guarded_allocations(0xFF, device_type='cpu'):
        assert all(getattr(torch, n) is not before[n] for n in names)
        assert torch.Tensor.new_empty is not meth['new_empty']
        with pytest.raises(AssertionError, match='does not nest'):
            with gd.guarded_allocations(0x5A, device_type='cpu'):
                pass
        assert all(getattr(torch, n) is not before[n] for n in names)  # the outer patches survive
    for n in names:
        assert getattr(torch, n) is before[n]
    with pytest.raises(KeyError):
        with gd.guarded_allocations(0x5A, device_type='cpu'):
            raise KeyError('body')
    for n in names:
        assert getattr(torch, n) is before[n]
    for n in own:
        assert (n in vars(torch.Tensor)) == own[n] and getattr(torch.Tensor, n) == meth[n]
    assert torch.ones(2).new_empty(3).shape == (3,)


def test_the_arena_keeps_every_backing_alive_and_counts():
    with gd.guarded_allocations(0x5A, device_type='cpu') as arena:
        for i in range(5):
            torch.empty(i, dtype=torch.float32, device='cpu')  # dropped at once by the caller
        assert arena.count == 5 and len(arena.allocs) == 5
        ptrs = {a.backing.data_ptr() for a in arena.allocs}
        assert len(ptrs) == 5  # none was recycled
