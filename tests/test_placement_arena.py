"""The arena of tests/_placement.py on CPU tensors: the proof, without a GPU, that tests/test_gpu_placement.py can fail -- a placement
is where it claims to be, an untouched arena passes, ONE planted value in front of a region, behind it or in the last guard byte is
found at the right offset, and a read that strays into an input's guard changes the result."""
import numpy as np
import pytest
import torch

import _placement as P

DTYPES = {"float32": (torch.float32, np.float32), "int32": (torch.int32, np.int32), "uint8": (torch.uint8, np.uint8), "int8": (torch.int8, np.int8)}


@pytest.mark.parametrize("byte_offset", [0, 4, 8, 12])
@pytest.mark.parametrize("n", [0, 1, 5, 1025])
def test_float_placements_are_where_they_claim(byte_offset, n):
    a = P.Arena(torch, P.need(4 * n, 4 * n))
    x = np.arange(n, dtype=np.float32) + 1
    t_in = a.place(x, torch.float32, byte_offset)
    t_out = a.place((n,), torch.float32, (byte_offset + 8) % 16)
    assert a.base % P.ALIGN == 0
    for t, off in ((t_in, byte_offset), (t_out, (byte_offset + 8) % 16)):
        assert t.is_contiguous() and t.dtype == torch.float32 and t.shape == (n,)
        if n:
            assert t.data_ptr() % 16 == off and (t.data_ptr() - a.base) % P.ALIGN == off
        before, after = a.guard_bytes(t) if n else (P.GUARD, P.GUARD)
        assert before >= P.GUARD and after >= P.GUARD
    assert np.array_equal(t_in.numpy(), x)
    if n:
        assert a.untouched(t_out) and (t_out.view(torch.int32) == P.CANARY).all()
    a.check()


@pytest.mark.parametrize("byte_offset", range(8))
def test_byte_placements_are_where_they_claim(byte_offset):
    a = P.Arena(torch, P.need(1003, 1003, 77))
    raw = np.random.default_rng(byte_offset).integers(0, 256, 1003, dtype=np.uint8)
    t_in = a.place(raw, torch.uint8, byte_offset)
    t_out = a.place((1003,), torch.uint8, 7 - byte_offset)
    t_have = a.place((77,), torch.int8, byte_offset)
    assert t_in.data_ptr() % 16 == byte_offset and t_out.data_ptr() % 16 == 7 - byte_offset and t_have.data_ptr() % 16 == byte_offset
    assert np.array_equal(t_in.numpy(), raw) and t_have.dtype == torch.int8
    assert a.untouched(t_out) and a.untouched(t_have)
    a.check()
    t_out[:] = 0
    assert not a.untouched(t_out)
    a.check()                                                  # writing the region itself is what an output is for


def test_a_misaligned_placement_is_refused():
    a = P.Arena(torch, P.need(64))
    with pytest.raises(AssertionError):
        a.place((16,), torch.float32, 2)                       # a float buffer needs 4-byte alignment: the header's promise, not less
    with pytest.raises(AssertionError):
        P.Arena(torch, 1000).place((16,), torch.float32, 0)    # (an arena that cannot hold the guards)


def test_shapes_and_arrays_with_more_dimensions():
    a = P.Arena(torch, P.need(4 * 700 * 2, 4 * 8 * 2 * 513 * 2))
    x = np.random.default_rng(1).uniform(-1, 1, (700, 2)).astype(np.float32)
    t = a.place(x, torch.float32, 12)
    o = a.place((8, 2, 513, 2), torch.float32, 4)
    assert t.shape == (700, 2) and o.shape == (8, 2, 513, 2) and o.is_contiguous() and o.data_ptr() % 16 == 4
    assert np.array_equal(t.numpy(), x)
    a.check()


def _plant(view):
    view.view(torch.uint8).fill_(0x01)                         # differs from every byte of both guard words


@pytest.mark.parametrize("output", [False, True])
@pytest.mark.parametrize("byte_offset", [0, 4, 12])
def test_one_planted_write_is_found_at_its_offset(output, byte_offset):
    n = 333
    x = np.ones(n, np.float32)

    def arena():
        a = P.Arena(torch, P.need(4 * n, 4 * n))
        other = a.place(x, torch.float32, 8)
        t = a.place((n,), torch.float32, byte_offset, name="victim") if output else a.place(x, torch.float32, byte_offset, name="victim")
        return a, t, other

    a, t, _ = arena()
    a.check()
    # one value in front of the region
    _plant(a.window(t, -1, 1))
    with pytest.raises(AssertionError, match=r"in front of 'victim' damaged: first byte at offset -4 "):
        a.check()
    # one value behind it
    a, t, _ = arena()
    _plant(a.window(t, n, 1))
    with pytest.raises(AssertionError, match=rf"behind 'victim' damaged: first byte at offset {4 * n} "):
        a.check()
    # the last byte of the guard behind it, and the first byte of the guard in front of it
    a, t, _ = arena()
    before, after = a.guard_bytes(t)
    _plant(a.bytes_at(t, 4 * n + after - 1, 1))
    with pytest.raises(AssertionError, match=rf"behind 'victim' damaged: first byte at offset {4 * n + after - 1} "):
        a.check()
    a, t, _ = arena()
    _plant(a.bytes_at(t, -before, 1))
    with pytest.raises(AssertionError, match=rf"in front of 'victim' damaged: first byte at offset {-before} "):
        a.check()
    # a write of 16 bytes that starts inside the region and runs over its end (a float4 store of a tail): the first byte behind
    a, t, _ = arena()
    _plant(a.window(t, n - 1, 4))
    with pytest.raises(AssertionError, match=rf"behind 'victim' damaged: first byte at offset {4 * n} "):
        a.check()
    # the region of ANOTHER buffer is not this region's guard: writes inside regions never trip the check
    a, t, other = arena()
    other.fill_(5.0)
    t.fill_(7.0)
    a.check()


@pytest.mark.parametrize("byte_offset", [1, 3, 6])
def test_planted_writes_around_a_byte_buffer(byte_offset):
    a = P.Arena(torch, P.need(1001))
    t = a.place((1001,), torch.uint8, byte_offset, name="bytes")
    a.check()
    _plant(a.bytes_at(t, 1001, 1))
    with pytest.raises(AssertionError, match=r"behind 'bytes' damaged: first byte at offset 1001 "):
        a.check()
    a = P.Arena(torch, P.need(1001))
    t = a.place((1001,), torch.uint8, byte_offset, name="bytes")
    _plant(a.bytes_at(t, -1, 1))
    with pytest.raises(AssertionError, match=r"in front of 'bytes' damaged: first byte at offset -1 "):
        a.check()


def test_the_canary_is_compared_as_bits_not_as_a_float():
    """both guard words are NaNs: a float comparison would call every guard damaged (NaN != NaN) or, with equal_nan, every NaN intact"""
    a = P.Arena(torch, P.need(64))
    t = a.place((16,), torch.float32, 4)
    assert torch.isnan(t).all() and a.untouched(t)
    a.window(t, 16, 1).view(torch.int32).fill_(P.NAN_BITS)     # another NaN behind an output: still damage
    with pytest.raises(AssertionError, match=r"offset 64 "):
        a.check()
    a = P.Arena(torch, P.need(64))
    t = a.place((16,), torch.float32, 4)
    t.view(torch.int32)[3] = P.NAN_BITS
    assert not a.untouched(t)
    with pytest.raises(AssertionError, match="never written"):
        a.assert_written(t)
    t.zero_()
    a.assert_written(t)


@pytest.mark.parametrize("byte_offset", [0, 4, 8, 12])
def test_a_read_into_the_guard_of_an_input_changes_a_reduction(byte_offset):
    n = 1000
    x = np.random.default_rng(3).uniform(-1, 1, n).astype(np.float32)
    a = P.Arena(torch, P.need(4 * n))
    t = a.place(x, torch.float32, byte_offset)
    assert float(t.sum()) == float(torch.from_numpy(x).sum())
    for first, count in ((0, n + 1), (-1, n + 1), (n - 3, 4)):           # one value too far at either end; a float4 over the end
        strayed = a.window(t, first, count)
        assert torch.isnan(strayed.sum()) and torch.isnan(strayed.abs().max())
    assert not torch.isnan(a.window(t, n - 4, 4).sum())
    a.check()                                                              # reading damages nothing
