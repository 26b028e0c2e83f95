"""CPU: the arenas of tests/buffer_lib.py have teeth.

The "kernel" here is a numpy function that fills a CPU arena's payload; each test gives it one defect of the
kind tests/test_caller_buffers.py exists to find on the device -- a store just outside the payload, a store
far outside it, an element that is never written, an input that is modified -- and wants the harness to
report it.  A correct stand-in passes at every offset and with both poisons.
"""
import numpy as np
import pytest

import buffer_lib as bl

N = 37  # elements; no multiple of anything
OFFSETS = (0, 1, 2, 3, 4, 8, 12, 255)


def whole(a):
    """the arena's whole allocation as numpy (CPU tensors share their memory)"""
    return a.buf.numpy()


def kernel(a_in, a_out, dtype, skip=None, stray=None, flip_input=None):
    """out[i] = in[i] for every i but `skip`; `stray` = a byte index relative to the payload of a_out that
    gets a store it should not; flip_input = a byte of the input that is changed"""
    src = whole(a_in)[a_in.start:a_in.end].view(dtype)
    dst = whole(a_out)[a_out.start:a_out.end].view(dtype)
    for i in range(src.size):
        if i != skip:
            dst[i] = src[i]
    if stray is not None:
        whole(a_out)[a_out.start + stray] ^= 0x5A
    if flip_input is not None:
        whole(a_in)[a_in.start + flip_input] ^= 0x01


def run(dtype, values, offset, poison, **defect):
    values = np.asarray(values, dtype)
    a_in = bl.arena_of(values, offset, poison, device="cpu")
    a_out = bl.arena(values.nbytes, offset, poison, device="cpu")
    bl.settle("cpu")
    kernel(a_in, a_out, dtype, **defect)
    a_out.check_equals(values, "out")
    a_in.check_input("in")


def run_both(dtype, values, offset=0, **defect):
    """-> the poisons under which the defect was reported"""
    caught = []
    for poison in bl.POISONS:
        try:
            run(dtype, values, offset, poison, **defect)
        except AssertionError as e:
            caught.append((poison, str(e)))
    return caught


def ramp(dtype):
    return (np.arange(N) * 7 + 1).astype(dtype)


def test_layout():
    for offset in OFFSETS:
        for poison in bl.POISONS:
            a = bl.arena(N * 4, offset, poison, device="cpu")
            assert a.payload.numel() == N * 4 and a.payload.is_contiguous()
            assert (a.ptr - offset) % 256 == 0
            assert a.payload.untyped_storage().data_ptr() == a.buf.untyped_storage().data_ptr(), "one allocation"
            assert a.start >= bl.GUARD and a.buf.numel() - a.end >= bl.GUARD
            w = whole(a)
            assert (w[:bl.GUARD] == bl.GUARD_BYTE).all() and (w[a.end:] == bl.GUARD_BYTE).all()
            assert (w[bl.GUARD:a.end] == poison).all() and bl.GUARD_BYTE != poison
            a.check_untouched()
            z = bl.arena_of(np.zeros(0, np.float32), offset, poison, device="cpu")  # n == 0: a valid address, no bytes
            assert (z.ptr - offset) % 256 == 0 and z.payload.numel() == 0
            z.check_input()
            z.check_untouched()
            if offset % 4 == 0:
                assert a.view(__import__("torch").float32, N).shape == (N,)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.uint8])
def test_correct_kernel_passes_at_every_offset(dtype, offset):
    assert run_both(dtype, ramp(dtype), offset) == []


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("stray,where", [(-1, "1 bytes before the payload"),
                                         (N * 4, "0 bytes past the payload's end"),
                                         (N * 4 + 60 * 1024, f"{60 * 1024} bytes past the payload's end"),
                                         (-60 * 1024, f"{60 * 1024} bytes before the payload")])
def test_stray_store_is_caught(offset, stray, where):
    caught = run_both(np.float32, ramp(np.float32), offset, stray=stray)
    assert [p for p, _ in caught] == list(bl.POISONS), "a stray store must show under either poison"
    assert all(where in msg for _, msg in caught), caught


@pytest.mark.parametrize("dtype,value", [(np.float32, 0), (np.int32, 0), (np.uint8, 0), (np.uint8, 205),
                                         (np.int32, -1), (np.uint8, 0x32), (np.float32, 1.5)])
@pytest.mark.parametrize("skip", [0, 17, N - 1])
def test_unwritten_element_is_caught_whatever_its_value(dtype, value, skip):
    values = ramp(dtype)
    values[skip] = value
    caught = run_both(dtype, values, skip=skip)
    assert caught, f"an element left unwritten (expected value {value}) passed under both poisons"
    assert all("out" in msg and "differ" in msg for _, msg in caught)
    # 205 = 0xCD hides under the first poison and 0x32 under the second: that is what the second run is for
    if dtype == np.uint8 and value in bl.POISONS:
        assert [p for p, _ in caught] == [p for p in bl.POISONS if p != value]


def test_zero_filled_buffers_would_have_missed_it():
    """the gap this harness closes: with a zeroed output an unwritten 0 equals its expected value"""
    values = ramp(np.float32)
    values[5] = 0
    out = np.zeros(N, np.float32)
    out[np.arange(N) != 5] = values[np.arange(N) != 5]
    assert np.array_equal(out, values)


@pytest.mark.parametrize("byte", [0, 3, N * 4 - 1])
def test_modified_input_is_caught(byte):
    caught = run_both(np.float32, ramp(np.float32), flip_input=byte)
    assert [p for p, _ in caught] == list(bl.POISONS)
    assert all("changed 1 input byte" in msg for _, msg in caught)


def test_elements_to_keep_must_hold_poison():
    """check_equals(keep=...): a byte the call must leave alone has to hold the poison still"""
    values = ramp(np.int32)
    keep = np.zeros(N * 4, bool)
    keep[8:12] = True  # element 2
    for poison in bl.POISONS:
        a = bl.arena(N * 4, 4, poison, device="cpu")
        dst = whole(a)[a.start:a.end].view(np.int32)
        dst[:] = values
        with pytest.raises(AssertionError):
            a.check_equals(values, keep=keep)  # it was written
        dst[2] = np.frombuffer(bytes([poison] * 4), np.int32)[0]
        a.check_equals(values, keep=keep)
        with pytest.raises(AssertionError):
            a.check_untouched()
        a.fill().check_untouched()


def test_refill_forgets_and_repoisons():
    a = bl.arena_of(ramp(np.float32), 8, bl.POISONS[1], device="cpu")
    a.check_input()
    whole(a)[a.start - 1] = 0
    with pytest.raises(AssertionError):
        a.check_guards()
    a.fill()
    a.check_untouched()
    with pytest.raises(AssertionError):
        a.check_input()  # nothing uploaded any more
