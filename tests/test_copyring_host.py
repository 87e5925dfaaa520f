"""x3d2_amd/copyring.py without a GPU, against a stand-in for the backend in the manner of checkpoint_ref.StubBackend: CPU
tensors, a copy that is made at once and counts as done when `landed` says so, a counter of the waits."""
import pytest
import torch

from x3d2_amd.common import X3dError
from x3d2_amd.copyring import CopyRing


class StubBackend:
    def __init__(self):
        self.landed = False  # True / False for every copy, or the set of the handles that are done
        self.waits = 0
        self.allocs = 0
        self.handles = 0

    def checkpoint_buffers(self, nbytes):
        self.allocs += 1
        return torch.zeros(nbytes, dtype=torch.uint8), torch.zeros(nbytes, dtype=torch.uint8)

    def snapshot_copy_async(self, host, dev, nbytes):
        host[:nbytes] = dev[:nbytes]
        self.handles += 1
        return self.handles

    def snapshot_done(self, handle):
        return handle in self.landed if isinstance(self.landed, set) else self.landed

    def snapshot_wait(self, handle):
        self.waits += 1


def pattern(k, n):
    return bytes((37 * k + 11 * i + 1) % 251 for i in range(n))


def make(nslot):
    b, seen = StubBackend(), []

    def on_land(payload, raw):
        seen.append((payload, raw.tobytes()))
        return payload

    ring = CopyRing(b, nslot, on_land)

    def send(k, nbytes=48, size=64):
        slot = ring.acquire(size)
        slot.dev[:nbytes] = torch.frombuffer(bytearray(pattern(k, nbytes)), dtype=torch.uint8)
        ring.submit(slot, nbytes, k)
        return slot

    return b, ring, seen, send


@pytest.mark.parametrize("nslot", [1, 2])
def test_ring_of_n_slots(nslot):
    b, ring, seen, send = make(nslot)
    # nothing before the first acquire
    assert ring.allocated == 0 and b.allocs == 0 and ring.pending() == [] and ring.poll() == [] and ring.drain() == []
    # round-robin, allocated as they are first handed out
    for k in range(nslot):
        assert send(k) is ring.slots[k] and ring.allocated == k + 1
    assert b.allocs == nslot and [p for _, p in ring.pending()] == list(range(nslot))
    # not landed: poll lands nothing and waits for nothing
    assert ring.poll() == [] and seen == [] and b.waits == 0 and ring.waits == 0
    # the (N+1)-th acquire: one wait, the oldest payload and its bytes, nothing else
    assert send(nslot) is ring.slots[0]
    assert b.waits == 1 and ring.waits == 1 and seen == [(0, pattern(0, 48))]
    assert [p for _, p in ring.pending()] == list(range(1, nslot + 1)) and b.allocs == nslot
    # landed: poll hands out the rest, oldest first, without a wait
    b.landed = True
    assert ring.poll() == list(range(1, nslot + 1)) and ring.poll() == [] and ring.pending() == []
    assert seen == [(k, pattern(k, 48)) for k in range(nslot + 1)] and b.waits == 1 and ring.waits == 1
    # drain: everything, oldest first, waiting for each; not a forced acquire
    b.landed = False
    for k in range(10, 10 + nslot):
        send(k)
    assert ring.drain() == list(range(10, 10 + nslot)) and ring.pending() == [] and ring.drain() == []
    assert b.waits == 1 + nslot and ring.waits == 1 and seen[-nslot:] == [(k, pattern(k, 48)) for k in range(10, 10 + nslot)]
    assert b.allocs == nslot and ring.allocated == nslot  # the same buffers all along


@pytest.mark.parametrize("nslot", [1, 2])
def test_a_larger_size_reallocates_an_idle_slot_and_never_a_pending_one(nslot):
    b, ring, seen, send = make(nslot)
    for k in range(nslot):
        send(k)
    ring.drain()
    small = ring.slots[0].dev
    slot = ring.acquire(16)  # smaller: the buffer stays
    assert slot is ring.slots[0] and slot.dev is small and b.allocs == nslot
    ring.submit(slot, 16, "small")
    for k in range(1, nslot):
        send(k)
    ring.drain()
    big = send(7, nbytes=100, size=128)  # idle and too small: new buffers
    assert big is ring.slots[0] and big.dev is not small and big.dev.numel() == big.host.numel() == 128
    assert b.allocs == nslot + 1 and ring.allocated == nslot
    for k in range(1, nslot):
        send(k)
    n = len(seen)
    held = big.dev
    again = ring.acquire(256)  # pending and too small: landed from the buffers it was submitted in, THEN replaced
    assert again is big and ring.waits == 1 and seen[n:] == [(7, pattern(7, 100))]
    assert again.dev is not held and again.dev.numel() == 256 and not again.pending and b.allocs == nslot + 2


def test_poll_stops_at_the_first_copy_that_is_not_done():
    b, ring, seen, send = make(2)
    first, second = send(0), send(1)
    b.landed = {second.handle}  # (cannot happen on one in-order stream; the ring must not reorder even so)
    assert ring.poll() == [] and seen == []
    b.landed = {first.handle}
    assert ring.poll() == [0] and [p for _, p in ring.pending()] == [1]
    b.landed = {first.handle, second.handle}
    assert ring.poll() == [1] and b.waits == 0


def test_land_one_slot_and_refuse_an_idle_one():
    b, ring, seen, send = make(2)
    first, second = send(0), send(1)
    assert ring.land(first) == 0 and b.waits == 1 and ring.waits == 0 and [p for _, p in ring.pending()] == [1]
    with pytest.raises(X3dError, match="no unlanded copy"):
        ring.land(first)
    assert ring.drain() == [1]
