"""Host-built device tables and status words on their way between the host and the device: the segment layout of an arena, the pinned staging
buffer with its fence (Staging), and the pinned read-back of status words (Mailbox).  The rules are written down in DESIGN.md, "Where a host-built
table travels"; optim.py's gradient-pointer table is the one deliberate exception."""
import torch

Event = torch.cuda.Event                                     # (module attributes, so that tests run the bookkeeping without a device)
_capturing = torch.cuda.is_current_stream_capturing


def layout(sizes):
    """Segments of `sizes` bytes one behind the other, each starting on a 16-byte boundary -> (offsets, total bytes)."""
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + 15) // 16 * 16
    return offs, total


def typed_views(segments):
    """segments: one (dtype, shape) each -> (views(buf) = the typed views of a uint8 buffer of `total` bytes, in segment order, total)."""
    sizes = [torch.empty(0, dtype=dt).element_size() * int(torch.Size(shape).numel()) for dt, shape in segments]
    offs, total = layout(sizes)

    def views(buf):
        return tuple(buf[o:o + n].view(dt).view(shape) for o, n, (dt, shape) in zip(offs, sizes, segments))

    return views, total


class Staging:
    """One host buffer that is filled and copied to fixed device addresses again and again, with its fence: the event recorded behind an upload's
    last copy, which the next open() waits for before the buffer is overwritten.
      open()            -> the host tensor, for writing (open_np(): its numpy view); the previous upload has left it
      upload((dst, src), ...) : dst.copy_(src, non_blocking=True) for every pair on the current stream -- src = the host tensor or slices / views of
                          it --, then ONE record (fence(): the record alone, for an owner that issues the copies itself).  Outside a capture.
    pin=None: pinned when `device` is a GPU.  A host-only instance (the CPU tests, packers that run in a loader) holds an ordinary tensor and has no
    fence: it constructs no event and needs no GPU runtime."""

    def __init__(self, host, device, pin=None):
        self.pinned = torch.device(device).type == "cuda" if pin is None else bool(pin)
        self.host = host.pin_memory() if self.pinned else host
        self._np = self.host.numpy()
        self._event = None

    def open(self):
        if self._event is not None:
            self._event.synchronize()          # the previous upload has left the staging buffer
        return self.host

    def open_np(self):
        self.open()
        return self._np

    def upload(self, *copies):
        for dst, src in copies:
            dst.copy_(src, non_blocking=True)
        self.fence()

    def upload_head(self, dst, n):
        """The first n elements alone, to the first n of `dst`: one copy of the part that was filled."""
        self.upload((dst[:n], self.host[:n]))

    def fence(self):
        """The record alone, behind copies out of the buffer that the caller has issued itself."""
        if self.pinned:
            if self._event is None:
                self._event = Event()
            self._event.record()


class Mailbox:
    """Status words read back without stalling the step: post() copies them to fresh pinned memory behind an event, drain() hands out the copies
    that have arrived.  What is raised for a word, in which order an owner posts and drains, and what stays queued after a raise are the owner's.
    `word`: the owner's sticky device word, when it keeps one.  It belongs to the owner's launches as the copies in flight do: a deep copy of the
    owner gets an empty mailbox without it."""

    def __init__(self):
        self._queue = []                       # (pinned host copy, event recorded behind the copy), oldest first
        self.word = None

    def __len__(self):
        return len(self._queue)

    def __deepcopy__(self, memo):
        return type(self)()

    def post(self, words):
        """Queue a copy of the device tensor `words`.  Nothing is queued for a host tensor, and nothing while the current stream is capturing (an
        event recorded on this stream before the capture may not even be queried then)."""
        if not words.is_cuda or _capturing():
            return
        host = torch.empty(words.shape, dtype=words.dtype, pin_memory=True)
        host.copy_(words, non_blocking=True)
        ev = Event()
        ev.record()
        self._queue.append((host, ev))

    def drain(self, wait=True, ordered=False):
        """Yield the host copies, oldest first, taking each out of the queue as it is yielded: all of them, each waited for (wait=True), or those
        that have arrived -- the others stay queued, in order.  ordered: stop at the first copy that has not arrived, for an owner whose copies
        mean something only in posting order.  A caller that stops midway leaves the rest queued; clear() drops them."""
        i = 0
        while i < len(self._queue):
            host, ev = self._queue[i]
            if wait or ev.query():
                del self._queue[i]
                ev.synchronize()
                yield host
            elif ordered:
                return
            else:
                i += 1

    def clear(self):
        del self._queue[:]
