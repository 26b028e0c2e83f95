"""Poisoned, guarded arenas for the buffers a test hands to a device entry point.

An arena is ONE torch.uint8 allocation laid out as

    [ front guard | pad up to a 256-byte boundary + offset | payload (nbytes) | back guard ]

The payload is what the call under test gets; the caller reinterprets it to the dtype it wants
(`Arena.view`).  Both guards are GUARD (64 KiB) long and hold GUARD_BYTE; the pad and the payload
hold the poison byte.  Because the guards and the pad are part of the payload's own allocation, a
store that strays up to 64 KiB before or behind the payload lands in memory the test owns and shows
up as a failed assertion in `check_guards`, not as a fault and not in a neighbour's block.

Two poisons.  Every case runs twice, with POISONS = (0xCD, 0x32).  What a call should have written
must equal the expected value in both runs; a byte it never wrote still holds the poison, and since
the two poisons differ that byte differs from its expected value in at least one run, whatever the
expected value is -- 0 (a black pixel, a miss), 0xFF (the bytes of -1) and 0xCD (205) included.
`both_poisons` is that loop.

Inputs live in arenas too (`upload`): after the call `check_input` wants the payload byte-identical
to what was uploaded and the guards and the pad intact.

Streams.  The renderer launches on its own stream and does not wait for torch's, so the fills and
uploads (torch's stream) must have finished before the call: `settle` synchronises torch's stream.
Reading back (`payload_bytes`, `check_guards`) copies on torch's stream, so the test synchronises
the renderer before it reads.

What this harness cannot see: a write further out than a guard (more than 64 KiB away from the
payload), and any out-of-bounds READ.

torch is imported inside the functions: the module itself imports without it.
"""
import numpy as np

GUARD = 64 * 1024
GUARD_BYTE = 0xA7
POISONS = (0xCD, 0x32)
ALIGN = 256


class Arena:
    def __init__(self, nbytes, offset=0, poison=POISONS[0], device="cuda"):
        import torch
        if not 0 <= offset < ALIGN:
            raise ValueError("offset must be in [0, 256)")
        if poison == GUARD_BYTE:
            raise ValueError("the poison must differ from the guard byte")
        self.nbytes, self.offset, self.poison = int(nbytes), int(offset), int(poison)
        total = GUARD + ALIGN + self.offset + self.nbytes + GUARD
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        self.start = (-(base + GUARD)) % ALIGN + GUARD + self.offset  # payload's index in buf
        self.end = self.start + self.nbytes
        self.payload = self.buf[self.start:self.end]
        self._ptr = base + self.start  # (an empty view has no address of its own)
        assert self.payload.is_contiguous() and (self.nbytes == 0 or self.payload.data_ptr() == self._ptr)
        assert (self._ptr - self.offset) % ALIGN == 0
        assert self.start >= GUARD and total - self.end >= GUARD
        self._uploaded = None
        self.fill()

    # ---- filling ------------------------------------------------------------------------------
    def fill(self):
        """(Re-)poison: guards to GUARD_BYTE, pad and payload to the poison byte; forgets an upload."""
        self.buf[:GUARD] = GUARD_BYTE
        self.buf[GUARD:self.end] = self.poison
        self.buf[self.end:] = GUARD_BYTE
        self._uploaded = None
        return self

    def upload(self, array):
        """Input data: the payload becomes the bytes of `array` (exactly nbytes of them)."""
        import torch
        raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        if raw.size != self.nbytes:
            raise ValueError(f"upload of {raw.size} bytes into a payload of {self.nbytes}")
        self._uploaded = raw.copy()
        self.payload.copy_(torch.from_numpy(self._uploaded))
        return self

    def view(self, dtype, *shape):
        """The payload as a contiguous tensor of `dtype` (shape: -1 when omitted).  A payload that is
        not aligned to the dtype cannot be viewed: pass `ptr` to the C ABI instead."""
        t = self.payload.view(dtype)
        return t.reshape(*shape) if shape else t

    @property
    def ptr(self):
        return self._ptr

    # ---- reading back -------------------------------------------------------------------------
    def payload_bytes(self):
        return self.payload.cpu().numpy().copy()

    def check_guards(self, what="buffer"):
        """Front guard, pad and back guard are as filled."""
        whole = self.buf.cpu().numpy()
        for name, lo, hi, byte in (("front guard", 0, GUARD, GUARD_BYTE),
                                   ("pad", GUARD, self.start, self.poison),
                                   ("back guard", self.end, whole.size, GUARD_BYTE)):
            bad = np.flatnonzero(whole[lo:hi] != byte)
            if bad.size:
                first = lo + int(bad[0]) - self.start
                rel = f"{-first} bytes before the payload" if first < 0 else \
                    f"{first - self.nbytes} bytes past the payload's end"
                raise AssertionError(f"{what}: {bad.size} stray byte(s) in the {name}, the first {rel} "
                                     f"(offset {self.offset}, poison {self.poison:#x})")

    def check_untouched(self, what="buffer"):
        """Nothing was written at all: the payload still holds its poison, the guards stand."""
        self.check_guards(what)
        bad = np.flatnonzero(self.payload_bytes() != self.poison)
        if bad.size:
            raise AssertionError(f"{what}: {bad.size} payload byte(s) written where none should be, the first "
                                 f"at byte {int(bad[0])} (offset {self.offset}, poison {self.poison:#x})")

    def check_input(self, what="input"):
        """An input is byte-identical to what was uploaded, and nothing around it changed."""
        if self._uploaded is None:
            raise AssertionError(f"{what}: check_input without an upload")
        self.check_guards(what)
        bad = np.flatnonzero(self.payload_bytes() != self._uploaded)
        if bad.size:
            raise AssertionError(f"{what}: the call changed {bad.size} input byte(s), the first at byte "
                                 f"{int(bad[0])} (offset {self.offset}, poison {self.poison:#x})")

    def check_equals(self, expected, what="output", keep=None):
        """The payload is, byte for byte, `expected` (a numpy array of nbytes bytes), and the guards stand.
        keep: a boolean mask over the BYTES of the payload that the call must leave alone -- those must
        still hold the poison, whatever `expected` says there."""
        self.check_guards(what)
        exp = np.ascontiguousarray(expected).reshape(-1).view(np.uint8)
        if exp.size != self.nbytes:
            raise AssertionError(f"{what}: expected value has {exp.size} bytes, the payload {self.nbytes}")
        if keep is not None:
            exp = np.where(np.asarray(keep).reshape(-1), np.uint8(self.poison), exp)
        got = self.payload_bytes()
        bad = np.flatnonzero(got != exp)
        if bad.size:
            b = int(bad[0])
            raise AssertionError(f"{what}: {bad.size} of {self.nbytes} bytes differ, the first at byte {b}: "
                                 f"got {int(got[b]):#x}, expected {int(exp[b]):#x} "
                                 f"(offset {self.offset}, poison {self.poison:#x})")


def arena(nbytes, offset=0, poison=POISONS[0], device="cuda"):
    return Arena(nbytes, offset, poison, device)


def arena_of(array, offset=0, poison=POISONS[0], device="cuda"):
    """An input arena holding the bytes of `array`."""
    a = np.ascontiguousarray(array)
    return Arena(a.nbytes, offset, poison, device).upload(a)


def settle(device="cuda"):
    """Fills and uploads ran on torch's stream; the renderer's stream does not wait for it."""
    import torch
    if torch.device(device).type == "cuda":
        torch.cuda.current_stream(torch.device(device)).synchronize()


def both_poisons(case):
    """Runs case(poison) once per poison.  Returns the results."""
    return [case(p) for p in POISONS]
