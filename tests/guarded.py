"""Guard-banded device buffers for the tests that check WHERE the engine writes.

Every buffer of one dtype is carved out of ONE torch allocation, with a band of at least BAND elements
before the first, between any two and behind the last, so a stray store of a few bytes (or of a whole
row) lands in memory the test owns and can inspect.  The bands and every output's interior are filled
with a recognisable pattern before the calls:

  fp64   a quiet NaN with a non-canonical payload (compared as int64 bits: the engine's own NaN rows of
         invalid EVs are the canonical NaN and differ from it)
  int8   0x5a (no LOMPC_QP_* value)
  int64  a fixed odd constant (no index)

Inputs are copied in from host arrays, which are kept: check_inputs compares the device bytes with them.
An fp64 input is followed by a band of NaN like every buffer, so a read past its end shows up as a NaN
result or N_INVALID != 0; padding INSIDE an input (strides larger than the record) is the caller's, who
fills it with NaN in the host array.  misalign = True starts every 8-byte buffer 8 bytes off a 16-byte
boundary (otherwise each starts on one).

    gb = Guarded()
    gb.inp("gamma", gn); gb.out("w", (B, N)); gb.out("status", (B,), torch.int8)
    gb.build()
    lib.lompc_plan_run(..., gb.ptr("w"), ...)
    gb.check_bands(); gb.check_written("w"); gb.check_inputs()
"""
import numpy as np
import torch

BAND = 4096
SENTINEL = {torch.float64: 0x7FF8DEAD0000BEEF, torch.int8: 0x5A, torch.int64: 0x5A5A5A5A5A5A5A5B}


def _bits(t):
    """The tensor's elements as integers (fp64 as int64 bits: NaN payloads compare)."""
    return t.view(torch.int64) if t.dtype == torch.float64 else t


class Guarded:
    def __init__(self, device="cuda:0", misalign=False):
        self.device, self.misalign = device, misalign
        self._spec = {}   # name -> (dtype, shape, host array or None)
        self._at = {}     # name -> (dtype, first element, elements)
        self._arena = {}  # dtype -> the allocation

    def out(self, name, shape, dtype=torch.float64):
        assert name not in self._spec and not self._arena
        self._spec[name] = (dtype, tuple(int(x) for x in shape), None)
        return self

    def inp(self, name, array):
        """An input: the host array is kept as the reference of check_inputs."""
        assert name not in self._spec and not self._arena
        a = np.ascontiguousarray(array)
        dtype = {np.dtype(np.float64): torch.float64, np.dtype(np.int64): torch.int64, np.dtype(np.int8): torch.int8}[a.dtype]
        self._spec[name] = (dtype, a.shape, a.copy())
        return self

    def build(self):
        for dtype in {s[0] for s in self._spec.values()}:
            item = torch.empty((), dtype=dtype).element_size()
            al = max(1, 16 // item)  # elements per 16 bytes
            pos = BAND
            for name, (dt, shape, _) in self._spec.items():
                if dt != dtype:
                    continue
                pos = (pos + al - 1) // al * al + (1 if self.misalign and item == 8 else 0)
                n = int(np.prod(shape, dtype=np.int64))
                self._at[name] = (dtype, pos, n)
                pos += n + BAND
            arena = torch.empty(pos, dtype=dtype, device=self.device)
            assert arena.data_ptr() % 16 == 0
            _bits(arena).fill_(SENTINEL[dtype])
            self._arena[dtype] = arena
        for name, (dt, shape, host) in self._spec.items():
            if host is not None:
                self.view(name).copy_(torch.as_tensor(host))
        if torch.device(self.device).type == "cuda":
            torch.cuda.synchronize()
        return self

    def view(self, name):
        """The buffer as a tensor of its shape (a view of the arena)."""
        dtype, a, n = self._at[name]
        return self._arena[dtype][a:a + n].view(self._spec[name][1])

    def ptr(self, name, offset=0):
        """Device address of element ``offset`` of the buffer (None for a name that was not declared)."""
        if name not in self._at:
            return None
        dtype, a, n = self._at[name]
        p = self._arena[dtype].data_ptr() + (a + offset) * self._arena[dtype].element_size()
        if dtype != torch.int8 and offset == 0:
            assert p % 8 == 0 and (p % 16 == 8) == self.misalign, (name, p)
        return p

    def np(self, name):
        return self.view(name).cpu().numpy()

    def _sentinel(self, name):
        return _bits(self.view(name)) == SENTINEL[self._at[name][0]]

    def check_bands(self):
        """Every element outside the declared buffers still holds the pattern, bit for bit."""
        for dtype, arena in self._arena.items():
            pos, bits = 0, _bits(arena)
            spans = sorted((a, n, name) for name, (dt, a, n) in self._at.items() if dt == dtype)
            for a, n, name in spans + [(arena.numel(), 0, "end")]:
                assert a - pos >= (BAND if name != "end" or spans else 0)
                bad = bits[pos:a] != SENTINEL[dtype]
                if bool(bad.any()):
                    k = torch.nonzero(bad).flatten()
                    raise AssertionError(f"{dtype} band before {name!r} modified at {int(bad.sum())} elements, offsets "
                                         f"{(k[:8] - (a - pos)).tolist()} relative to its start")
                pos = a + n

    def check_written(self, name, mask=None):
        """No pattern left inside the output (mask: only where it is True, and the pattern must REMAIN
        everywhere else — gap rows between strided runs)."""
        left = self._sentinel(name)
        if mask is None:
            assert not bool(left.any()), f"{name}: {int(left.sum())} elements never written"
            return
        m = torch.as_tensor(np.broadcast_to(mask, left.shape).copy(), device=left.device)
        assert not bool((left & m).any()), f"{name}: {int((left & m).sum())} elements never written"
        assert bool((left | m).all()), f"{name}: {int((~(left | m)).sum())} gap elements modified"

    def check_untouched(self, name):
        """The whole buffer still holds the pattern (an output the call must not write)."""
        left = self._sentinel(name)
        assert bool(left.all()), f"{name}: {int((~left).sum())} elements modified"

    def check_inputs(self):
        """Every input is bitwise its host copy."""
        for name, (dt, shape, host) in self._spec.items():
            if host is not None:
                same = torch.equal(_bits(self.view(name)), _bits(torch.as_tensor(host)).to(self.device))
                assert same, f"input {name} modified"
