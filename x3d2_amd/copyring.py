"""CopyRing: the one way results leave the device asynchronously (snapshots, checkpoints, the diagnostics series).

A ring of N slots, each a device byte buffer and its pinned host twin.  The owner acquires the next slot, fills its
device buffer, and submits it with a payload of its own: ONE asynchronous copy into the twin on the copy stream
(HipBackend.snapshot_copy_async).  A copy is `landed` by handing (payload, host bytes) to the owner's callback: by poll()
once it is done, never waiting; by drain() and land(), which wait for it.  The (N+1)-th acquire before the first copy was
landed waits for it, lands it, and counts `waits`.

The copies of one backend share one in-order stream, so an older copy that is not done implies a newer one that is not:
everything here goes oldest first.  The library keys its copy events by device pointer and has 16 per backend
(X3D_SNAP_SLOTS): a slot is reallocated only when a larger size is asked for, and never while its copy is unlanded.  The
rings of one backend together: Snapshots 2, Checkpoints 1, Diagnostics, Loads, Probes and Particles 2 each -- 11 with all
attached."""
from .common import X3dError


class Slot:
    """dev, host: the two buffers (None until first acquired); pending: submitted and not landed yet"""
    dev = host = handle = payload = None
    nbytes = 0
    pending = False


class CopyRing:
    """CopyRing(backend, nslot, on_land): on_land(payload, host_bytes) lands one copy, host_bytes being the submitted
    bytes as a numpy uint8 view of the pinned buffer (valid until the slot is acquired again); what it returns is what
    poll() and drain() collect"""

    def __init__(self, backend, nslot, on_land):
        self.backend, self.on_land = backend, on_land
        self.slots = [Slot() for _ in range(int(nslot))]
        self.waits = 0  # acquires that had to wait for their slot's previous copy
        self._next = 0  # the slot the next acquire hands out: the oldest

    @property
    def allocated(self):
        """the number of slots that hold buffers: 0 until the first acquire"""
        return sum(s.dev is not None for s in self.slots)

    def acquire(self, nbytes):
        """the next slot, round-robin, with buffers of at least nbytes (zero-filled on the device when new)"""
        slot = self.slots[self._next]
        self._next = (self._next + 1) % len(self.slots)
        if slot.pending:
            self.waits += 1
            self.land(slot)
        if slot.dev is None or slot.dev.numel() < nbytes:
            slot.dev, slot.host = self.backend.checkpoint_buffers(nbytes)
        return slot

    def submit(self, slot, nbytes, payload):
        """start the copy of the first nbytes of slot.dev, ordered behind what is queued on the compute stream"""
        slot.handle = self.backend.snapshot_copy_async(slot.host, slot.dev, nbytes)
        slot.nbytes, slot.payload, slot.pending = int(nbytes), payload, True

    def pending(self):
        """[(slot, payload)] of the unlanded copies, oldest first"""
        n = len(self.slots)
        order = (self.slots[(self._next + i) % n] for i in range(n))
        return [(s, s.payload) for s in order if s.pending]

    def _deliver(self, slot):
        payload, slot.payload, slot.pending = slot.payload, None, False
        return self.on_land(payload, slot.host.numpy()[:slot.nbytes])

    def land(self, slot):
        """wait for the slot's copy (at once if it is done; counted by the backend's sync_count) and land it"""
        if not slot.pending:
            raise X3dError("CopyRing.land: the slot has no unlanded copy")
        self.backend.snapshot_wait(slot.handle)
        return self._deliver(slot)

    def poll(self):
        """land the copies that are done, oldest first, up to the first that is not; never waits"""
        out = []
        for slot, _ in self.pending():
            if not self.backend.snapshot_done(slot.handle):
                break
            out.append(self._deliver(slot))
        return out

    def drain(self):
        """land everything, oldest first, waiting for each"""
        return [self.land(slot) for slot, _ in self.pending()]
