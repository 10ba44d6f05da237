"""Caller buffers at chosen byte offsets, between guard zones -- TEST INFRASTRUCTURE ONLY (plain module, like _oracle.py).

The C ABI takes plain device pointers and promises that a buffer needs only the alignment of its element type and that nothing
outside it is read or written (include/awm_hip.h).  A fresh torch allocation cannot test that: it is at least 512-byte aligned and
has allocator slack behind it.  An Arena is ONE allocation (uint8, used from a base rounded up to 256 bytes) in which every buffer
of a call is placed at  base + k * 256 + byte_offset  with at least GUARD bytes of guard zone in front of it and behind it:

  inputs   guards of float32 NaNs (0x7fc00000, phased to the region's ends): a read past either end that reaches the arithmetic
           shows in the result, which the tests compare bit for bit with the result at an aligned placement;
  outputs  guards -- and the region itself until the call writes it -- of the 32-bit canary 0x7fc0beef, a NaN with a payload that
           no kernel produces.  check() compares every guard bit for bit (as integers, never as floats: NaN != NaN) and names the
           first damaged byte relative to the region: negative in front of it, >= the region's size behind it.

Everything works on CPU tensors too; that is how tests/test_placement_arena.py proves, without a GPU, that the GPU tests can fail."""
import numpy as np

GUARD = 64 * 1024            # bytes of guard zone on either side of a region, at least
ALIGN = 256                  # the arena's base, and the grid the byte offsets are relative to
NAN_BITS = 0x7FC00000        # guards of inputs
CANARY = 0x7FC0BEEF          # guards of outputs and the unwritten output itself


def _round_up(n, to):
    return (n + to - 1) // to * to


def need(*region_bytes):
    """arena capacity for regions of these sizes in bytes, at any byte offset below ALIGN"""
    return sum(_round_up(int(n) + ALIGN, ALIGN) + 2 * GUARD + ALIGN for n in region_bytes) + ALIGN


def _pattern(bits, length, phase):
    """`length` bytes of the little-endian 32-bit word `bits` repeated, the first byte being byte `phase % 4` of the word"""
    word = np.frombuffer(np.uint32(bits).tobytes(), np.uint8)
    reps = (length + (phase % 4) + 3) // 4 + 1
    return np.tile(word, reps)[phase % 4: phase % 4 + length]


class _Region:
    __slots__ = ("name", "start", "nbytes", "before", "after", "bits", "is_output")


class Arena:
    def __init__(self, torch, capacity_bytes, device="cpu"):
        self.torch = torch
        self.raw = torch.zeros(int(capacity_bytes) + ALIGN, dtype=torch.uint8, device=device)       # the one allocation
        self.base_off = (-self.raw.data_ptr()) % ALIGN
        self.base = self.raw.data_ptr() + self.base_off
        self.capacity = int(capacity_bytes)
        self.cursor = 0                          # next free byte relative to base, a multiple of ALIGN
        self.regions = {}                        # data_ptr of the region -> _Region

    # -- layout ------------------------------------------------------------------------------------------------------------
    def _bytes(self, start, count):
        return self.raw[self.base_off + start: self.base_off + start + count]

    def _fill(self, start, count, bits, phase):
        if count:
            self._bytes(start, count).copy_(self.torch.from_numpy(_pattern(bits, count, phase).copy()))

    def place(self, array_or_shape, dtype, byte_offset, output=None, name=None):
        """A contiguous tensor view of `dtype` (a torch dtype) whose data_ptr() is base + k * 256 + byte_offset.
        An array (numpy) is copied in and is an INPUT (NaN guards) unless output=True (a buffer the call updates in place: canary
        guards, the array's values inside); a shape is an OUTPUT: canary guards, and canaries inside until somebody writes it."""
        torch = self.torch
        is_array = isinstance(array_or_shape, np.ndarray)
        if output is None:
            output = not is_array
        shape = tuple(array_or_shape.shape) if is_array else ((array_or_shape,) if isinstance(array_or_shape, int) else tuple(array_or_shape))
        itemsize = torch.empty(0, dtype=dtype).element_size()
        assert 0 <= byte_offset < ALIGN and byte_offset % itemsize == 0, "a buffer needs the alignment of its element type"
        count = int(np.prod(shape, dtype=np.int64))
        nbytes = count * itemsize
        r = _Region()
        r.name = name or ("out" if output else "in") + str(len(self.regions))
        r.start = self.cursor + GUARD + byte_offset
        r.nbytes = nbytes
        r.before = GUARD + byte_offset
        end = r.start + nbytes
        nxt = _round_up(end + GUARD, ALIGN)
        r.after = nxt - end
        r.bits = CANARY if output else NAN_BITS
        r.is_output = output
        assert nxt <= self.capacity, f"arena too small: {nxt} > {self.capacity} bytes (size it with need())"
        self._fill(self.cursor, r.before, r.bits, -r.before)                # ends with a whole word right in front of the region
        self._fill(end, r.after, r.bits, 0)                                 # starts with a whole word right behind it
        view = self._bytes(r.start, nbytes).view(dtype).reshape(shape)
        if is_array:
            a = np.ascontiguousarray(array_or_shape)
            assert a.dtype.itemsize == itemsize, (a.dtype, dtype)
            if nbytes:
                view.copy_(torch.from_numpy(a).to(view.device).view(dtype))
        else:
            self._fill(r.start, nbytes, CANARY, 0)
        assert view.is_contiguous() and (nbytes == 0 or view.data_ptr() == self.base + r.start)
        self.cursor = nxt
        self.regions[self.base + r.start] = r
        return view

    def _region(self, t):
        return self.regions[t.data_ptr()] if not isinstance(t, _Region) else t

    # -- access around a region (self-tests: planted writes and reads) --------------------------------------------------------
    def bytes_at(self, t, rel_byte, count):
        """uint8 view of `count` bytes starting `rel_byte` bytes from the region's first byte (negative: the guard in front)"""
        r = self._region(t)
        assert -r.before <= rel_byte and rel_byte + count <= r.nbytes + r.after
        return self._bytes(r.start + rel_byte, count)

    def window(self, t, first, count):
        """view of t's dtype over `count` elements starting `first` elements from the region's first one: what a kernel that runs
        past an end would touch"""
        size = t.element_size()
        return self.bytes_at(t, first * size, count * size).view(t.dtype)

    def guard_bytes(self, t):
        r = self._region(t)
        return r.before, r.after

    # -- checks ------------------------------------------------------------------------------------------------------------
    def _first_damage(self, start, count, bits, phase):
        got = self._bytes(start, count)
        want = self.torch.from_numpy(_pattern(bits, count, phase).copy()).to(got.device)
        if self.torch.equal(got, want):
            return None
        return int((got != want).nonzero()[0, 0])

    def check(self):
        """every guard bit for bit intact; AssertionError names the region and the first damaged byte offset relative to it"""
        for r in self.regions.values():
            k = self._first_damage(r.start - r.before, r.before, r.bits, -r.before)
            if k is not None:
                raise AssertionError(f"guard in front of '{r.name}' damaged: first byte at offset {k - r.before} of the region")
            k = self._first_damage(r.start + r.nbytes, r.after, r.bits, 0)
            if k is not None:
                raise AssertionError(f"guard behind '{r.name}' damaged: first byte at offset {r.nbytes + k} of the region ({r.nbytes} bytes)")

    def untouched(self, t):
        """an output nobody wrote: still canaries (compared as int32 where the region is made of whole words)"""
        r = self._region(t)
        assert r.is_output
        if r.nbytes % 4 == 0 and r.start % 4 == 0 and r.nbytes:
            words = self._bytes(r.start, r.nbytes).view(self.torch.int32)
            return bool((words == CANARY).all())
        return self._first_damage(r.start, r.nbytes, CANARY, 0) is None

    def assert_written(self, t):
        """an output of 32-bit elements that a call claims to have filled holds no canary any more"""
        r = self._region(t)
        assert r.is_output and r.nbytes % 4 == 0 and r.start % 4 == 0
        if r.nbytes:
            words = self._bytes(r.start, r.nbytes).view(self.torch.int32)
            left = int((words == CANARY).sum())
            assert left == 0, f"'{r.name}': {left} of {r.nbytes // 4} words were never written"
