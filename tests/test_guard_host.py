"""The guard harness of tests/guard.py, tested on CPU tensors: what it must catch is made to happen here, in host memory and through
the slab's own tensor, and nowhere else.  The stand-in "ops" are a few lines of torch / NumPy."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from astrophotography_amd import _lib, ops

from tests.guard import (CANARY, MIN_GUARD, STREAM_LAST, GuardedTorch, OPS_CACHES, RecordingLib, current, guard_width, guarded, intact,
                   place, unchanged)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def raw_bytes(t):
    """All bytes of the storage behind a view, the guards included (the way a stray pointer sees them)."""
    return torch.tensor([], dtype=torch.uint8).set_(t.untyped_storage())


def first_byte(t):
    return t.storage_offset() * t.element_size()


def fake_op_scale(gt, x):
    """A well-behaved op: allocates its output and a workspace like ops.py does and stays inside both."""
    out = gt.empty_like(x)
    ws = gt.empty(x.numel() * 4, dtype=torch.uint8, device=x.device)
    ws.zero_()
    out.copy_(x * 2)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
def test_check_passes_when_the_op_stays_inside():
    gt = GuardedTorch(512)
    x = torch.arange(7 * 9, dtype=torch.float32).reshape(7, 9)
    out = fake_op_scale(gt, x)
    assert torch.equal(out, x * 2)
    assert len(gt.allocations) == 2
    gt.check()


@pytest.mark.parametrize('make, what', [
    (lambda gt: gt.empty((5, 3), dtype=torch.float32, device='cpu'), 'empty([5, 3], float32)'),
    (lambda gt: gt.empty_like(torch.zeros(7, dtype=torch.float64)), 'empty_like([7], float64)'),
    (lambda gt: gt.zeros(3, dtype=torch.int64, device='cpu'), 'zeros([3], int64)'),
])
@pytest.mark.parametrize('side', ['after', 'before'])
def test_check_fails_one_byte_outside(make, what, side):
    gt = GuardedTorch(1024)
    gt.empty(16, dtype=torch.uint8, device='cpu')                  # a neighbour that stays intact and must not be named
    t = make(gt)
    line = make.__code__.co_firstlineno
    nbytes = t.numel() * t.element_size()
    raw = raw_bytes(t)
    at = first_byte(t) + (nbytes if side == 'after' else -1)
    assert raw[at] == CANARY
    raw[at] = 0
    with pytest.raises(AssertionError) as e:
        gt.check()
    msg = str(e.value)
    expect = "canary %s %s at test_guard_host.py:%d damaged: 1 byte(s), first at offset %s from the tensor's %s" % (
        side, what, line, '+0' if side == 'after' else '-1', 'end' if side == 'after' else 'start')
    assert msg == expect


def test_check_reports_extent_of_an_overrun():
    gt = GuardedTorch(512)
    t = gt.empty(6, dtype=torch.float32, device='cpu')
    raw_bytes(t)[first_byte(t) + 24:first_byte(t) + 24 + 16] = 1   # a float4 store that begins at the last element + 1
    with pytest.raises(AssertionError, match=r"canary after empty\(\[6\], float32\) at test_guard_host\.py:\d+ damaged: 16 byte\(s\), "
                                             r"first at offset \+0 from the tensor's end"):
        gt.check()


def test_the_canary_begins_at_the_first_byte_after_the_tensor():
    gt = GuardedTorch(512)
    for n in (1, 2, 3, 5, 511, 513):
        t = gt.empty(n, dtype=torch.uint8, device='cpu')
        raw = raw_bytes(t)
        assert raw.numel() == 512 + n + 512
        t.fill_(0)
        assert (raw[:512] == CANARY).all() and (raw[512 + n:] == CANARY).all() and (raw[512:512 + n] == 0).all()
    gt.check()


# the forms of ops.py's allocation calls (grep "torch\.(empty|zeros|ones|empty_like|full_like)\(" astrophotography_amd/ops.py): a shape
# tuple, a torch.Size (raw.shape, slab.shape[1:]), a tuple sum ((3,) + shp), one int, an empty dimension (n = 0 candidates), dtype= and
# device= keywords, dtype= alone (the host tensor of _oversampling_args).  Several ints as varargs do not occur; torch takes them, so
# does the proxy.
FORMS = [
    ('tuple', lambda t: t.empty((4, 5), dtype=torch.float32, device='cpu'), (4, 5), torch.float32),
    ('size', lambda t: t.empty(torch.zeros(2, 3, 4).shape, dtype=torch.float64, device='cpu'), (2, 3, 4), torch.float64),
    ('size_slice', lambda t: t.empty(torch.zeros(2, 3, 4).shape[1:], dtype=torch.float32, device='cpu'), (3, 4), torch.float32),
    ('tuple_sum', lambda t: t.empty((3,) + (6, 7), dtype=torch.float32, device='cpu'), (3, 6, 7), torch.float32),
    ('int', lambda t: t.empty(10, dtype=torch.float64, device='cpu'), (10,), torch.float64),
    ('int_u8', lambda t: t.empty(1001, dtype=torch.uint8, device='cpu'), (1001,), torch.uint8),
    ('numpy_int', lambda t: t.empty(np.int64(6), dtype=torch.int32, device='cpu'), (6,), torch.int32),
    ('empty_dim', lambda t: t.empty((0, 16), dtype=torch.float64, device='cpu'), (0, 16), torch.float64),
    ('u16', lambda t: t.empty((4, 6, 5), dtype=torch.uint16, device='cpu'), (4, 6, 5), torch.uint16),
    ('u64', lambda t: t.empty(4, dtype=torch.uint64, device='cpu'), (4,), torch.uint64),
    ('device_object', lambda t: t.empty((2, 2), dtype=torch.int32, device=torch.device('cpu')), (2, 2), torch.int32),
    ('dtype_only', lambda t: t.ones(5, dtype=torch.float32), (5,), torch.float32),
    ('varargs', lambda t: t.empty(2, 3, dtype=torch.float32, device='cpu'), (2, 3), torch.float32),
    ('default_dtype', lambda t: t.empty((2, 3)), (2, 3), torch.float32),
    ('zeros_tuple', lambda t: t.zeros((3, 20), dtype=torch.float64, device='cpu'), (3, 20), torch.float64),
    ('zeros_int', lambda t: t.zeros(1, dtype=torch.int64, device='cpu'), (1,), torch.int64),
    ('empty_like', lambda t: t.empty_like(torch.zeros((3, 5), dtype=torch.uint8)), (3, 5), torch.uint8),
    ('full_like', lambda t: t.full_like(torch.zeros((3, 5), dtype=torch.float32), float('nan')), (3, 5), torch.float32),
]


@pytest.mark.parametrize('name, make, shape, dtype', FORMS, ids=[f[0] for f in FORMS])
def test_call_forms(name, make, shape, dtype):
    G = 1536
    gt = GuardedTorch(G)
    t = make(gt)
    same = make(torch)
    assert tuple(t.shape) == shape == tuple(same.shape) and t.dtype == dtype == same.dtype and t.device == same.device
    assert t.is_contiguous() and t.stride() == same.stride()
    assert first_byte(t) == G and G % 512 == 0                      # 512-byte aligned relative to the slab
    assert raw_bytes(t).numel() == 2 * G + t.numel() * t.element_size()
    gt.check()


def test_unknown_keywords_are_refused():
    with pytest.raises(TypeError, match='pin_memory'):
        GuardedTorch(512).empty(4, dtype=torch.uint8, pin_memory=True)
    with pytest.raises(ValueError, match='multiple of 512'):
        GuardedTorch(100)


def test_fills_inside_and_canary_outside():
    gt = GuardedTorch(512)
    z = gt.zeros((3, 5), dtype=torch.float32, device='cpu')
    o = gt.ones(7, dtype=torch.float32)
    f = gt.full_like(z, 2.5)
    n = gt.full_like(z, float('nan'))
    assert (z == 0).all() and (o == 1).all() and (f == 2.5).all() and torch.isnan(n).all()
    for t in (z, o, f, n):
        raw, lo = raw_bytes(t), first_byte(t)
        hi = lo + t.numel() * t.element_size()
        assert (raw[:lo] == CANARY).all() and (raw[hi:] == CANARY).all()
    assert (raw_bytes(z)[512:512 + 60] == 0).all()
    gt.check()


def test_everything_else_is_torch():
    gt = GuardedTorch(512)
    assert gt.float32 is torch.float32 and gt.from_numpy is torch.from_numpy and gt.cuda is torch.cuda
    assert gt.is_tensor(gt.empty(1, dtype=torch.uint8))


def test_guard_width():
    assert guard_width() == MIN_GUARD == 65536 and guard_width(1032 * 4) == 65536
    assert guard_width(8193 * 8) == 262656 and guard_width(8193 * 8) % 512 == 0 and guard_width(8193 * 8) >= 4 * 8193 * 8


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64, np.uint16, np.uint8, np.int32])
@pytest.mark.parametrize('shifted', [False, True])
def test_place_and_unchanged(dtype, shifted):
    a = (np.arange(7 * 9) % 251).astype(dtype).reshape(7, 9)
    shift = a.dtype.itemsize if shifted else 0
    t, tok = place(a, 0xFF, shift, guard=512, device='cpu')
    assert tuple(t.shape) == a.shape and t.is_contiguous()
    assert first_byte(t) == 512 + shift and first_byte(t) % 16 == shift
    assert np.array_equal(current(tok).view(dtype).reshape(a.shape), a)
    raw = raw_bytes(t)
    assert raw.numel() == 1024 + shift + a.nbytes and (raw[:512 + shift] == 0xFF).all() and (raw[512 + shift + a.nbytes:] == 0xFF).all()
    unchanged(tok)
    intact(tok)


def test_place_refuses_other_shifts():
    with pytest.raises(ValueError, match='shift must be 0 or one element'):
        place(np.zeros(4, np.float32), 0, 2, guard=512, device='cpu')


def test_unchanged_fails_for_one_input_byte():
    t, tok = place(np.arange(12, dtype=np.float32), 0x00, guard=512, device='cpu')
    raw_bytes(t)[first_byte(t) + 13] ^= 1
    with pytest.raises(AssertionError) as e:
        unchanged(tok)
    assert str(e.value) == 'input was written: 1 byte(s) changed, first at byte 13'
    intact(tok)                                                     # the surround is whole: an output may change like this


@pytest.mark.parametrize('side, at, text', [('after', 48, '+0 from its end'), ('before', -1, '-1 from its start'),
                                            ('after', 48 + 511, '+511 from its end'), ('before', -512, '-512 from its start')])
@pytest.mark.parametrize('poison', [0x00, 0xFF])
def test_unchanged_fails_for_one_surround_byte(side, at, text, poison):
    t, tok = place(np.arange(12, dtype=np.float32), poison, guard=512, device='cpu', what='input dark')
    raw_bytes(t)[first_byte(t) + at] = 0x5A
    for fn in (unchanged, intact):
        with pytest.raises(AssertionError) as e:
            fn(tok)
        assert str(e.value) == 'surround %s input dark damaged: 1 byte(s), first at offset %s' % (side, text)


# ---------------------------------------------------------------------------------------------------------------------------
class FakeLib:
    """A small stand-in for the loaded library: three entry points named like the real ones, and one other attribute."""

    def __init__(self):
        self.seen = []
        self.other = 'not a function of the ABI'

    def apgpu_version(self):
        self.seen.append(('apgpu_version',))
        return 7

    def apgpu_deconv_ws_bytes(self, h, w):
        self.seen.append(('apgpu_deconv_ws_bytes', h, w))
        return 16 * h * w

    def apgpu_linear_combine_f32(self, *args):
        self.seen.append(('apgpu_linear_combine_f32',) + args)
        return 0

    def apgpu_last_error(self):
        return b''


def test_recording_wrapper_notes_names_and_streams():
    fake = FakeLib()
    rec = RecordingLib(fake)
    assert rec.apgpu_version() == 7 and rec.apgpu_deconv_ws_bytes(3, 5) == 240
    assert rec.other == fake.other
    x = C.c_void_p(4096)
    assert rec.apgpu_linear_combine_f32(x, None, 1.0, 0.0, 0.0, x, 12, C.c_void_p(0xBEEF0)) == 0
    rec.apgpu_linear_combine_f32(x, None, 1.0, 0.0, 0.0, x, 12, C.c_void_p(0))           # the default stream: ctypes makes it None
    rec.apgpu_linear_combine_f32(x, None, 1.0, 0.0, 0.0, x, 12, None)
    rec.apgpu_linear_combine_f32(x, None, 1.0, 0.0, 0.0, x, 12, 77)
    assert rec.calls == [('apgpu_version', None), ('apgpu_deconv_ws_bytes', None), ('apgpu_linear_combine_f32', 0xBEEF0),
                         ('apgpu_linear_combine_f32', 0), ('apgpu_linear_combine_f32', 0), ('apgpu_linear_combine_f32', 77)]
    assert rec.names() == {'apgpu_version', 'apgpu_deconv_ws_bytes', 'apgpu_linear_combine_f32'}
    assert rec.streams() == [('apgpu_linear_combine_f32', s) for s in (0xBEEF0, 0, 0, 77)]
    assert [s[0] for s in fake.seen] == [c[0] for c in rec.calls]   # every call went through, in order
    assert fake.seen[2][1:] == (x, None, 1.0, 0.0, 0.0, x, 12) + fake.seen[2][-1:] and fake.seen[2][-1].value == 0xBEEF0
    with pytest.raises(AttributeError):
        rec.apgpu_no_such_function


def test_stream_functions_are_those_of_the_header():
    """STREAM_LAST (last argtype c_void_p in _lib.SIGNATURES) against include/apgpu.h: exactly the prototypes that end in
    `void *stream`, and every prototype of the header is in SIGNATURES."""
    text = open(os.path.join(ROOT, 'include', 'apgpu.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'//[^\n]*', '', text)
    protos = dict(re.findall(r'\b(apgpu_\w+)\s*\(([^;{}]*?)\)\s*;', text))
    assert set(protos) == set(_lib.SIGNATURES)
    with_stream = {n for n, args in protos.items() if re.search(r'void\s*\*\s*stream\s*$', args.strip())}
    assert with_stream == set(STREAM_LAST) and len(with_stream) > 50


# ---------------------------------------------------------------------------------------------------------------------------
def test_guarded_swaps_and_restores(monkeypatch):
    fake = FakeLib()
    real_lib = object()
    monkeypatch.setattr(_lib, '_lib', real_lib)                     # stands for the loaded library; never called
    cached = {name: {('dev', 0, 1): torch.zeros(3)} for name in OPS_CACHES}
    for name in OPS_CACHES:
        assert isinstance(getattr(ops, name), dict)
        monkeypatch.setattr(ops, name, cached[name])
    with guarded(monkeypatch, guard=512, lib=fake) as g:
        assert ops.torch is g.torch and isinstance(g.torch, GuardedTorch)
        assert _lib.load() is g.lib and isinstance(g.lib, RecordingLib)
        for name in OPS_CACHES:
            assert getattr(ops, name) == {} and getattr(ops, name) is not cached[name]
        ops._stack_ws['x'] = 1                                      # what a call caches under the guard does not outlive it
        # ops.py itself now allocates through the proxy and calls through the recorder
        out = ops._out_f32(None, torch.zeros((3, 4), dtype=torch.float32))
        assert first_byte(out) == 512 and g.torch.allocations[-1].site.startswith('ops.py:')
        _lib.check(_lib.load().apgpu_linear_combine_f32(1, 2, C.c_void_p(5)))
        assert g.lib.calls == [('apgpu_linear_combine_f32', 5)]
    assert ops.torch is torch and _lib._lib is real_lib
    for name in OPS_CACHES:
        assert getattr(ops, name) is cached[name] and len(cached[name]) == 1


def test_guarded_checks_on_exit(monkeypatch):
    monkeypatch.setattr(_lib, '_lib', object())
    with pytest.raises(AssertionError, match=r"canary after empty_like\(\[3, 4\], float32\) at ops\.py:\d+ damaged: 4 byte\(s\), first at "
                                             r"offset \+0 from the tensor's end"):
        with guarded(monkeypatch, guard=512, lib=FakeLib()):
            out = ops._out_f32(None, torch.zeros((3, 4), dtype=torch.float32))
            raw_bytes(out)[first_byte(out) + 48:first_byte(out) + 52] = 0           # one float32 past the end
    assert ops.torch is torch


def test_guarded_restores_after_an_error(monkeypatch):
    marker = object()
    monkeypatch.setattr(_lib, '_lib', marker)
    with pytest.raises(KeyError):
        with guarded(monkeypatch, guard=512, lib=FakeLib()):
            raise KeyError('the case failed')
    assert ops.torch is torch and _lib._lib is marker
