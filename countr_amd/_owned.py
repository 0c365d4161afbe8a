"""What the wrapper classes that own device buffers have in common, each rule stated once: the device they are made for, the one
instance per device, the buffers that only grow, the guard of a call from another stream, and the stream handle of a launch."""
import ctypes as C

from ._lib import CountrError

_instances = {}             # (class, resolved device) -> its instance


def _indexed(device):
    """torch.device(device); a plain "cuda" is the calling thread's current device (rank k of a multi-GPU job), not 0."""
    import torch
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def resolve(device, who):
    """The device of a wrapper of class `who`, with its index; anything but a GPU raises."""
    device = _indexed(device)
    if device.type != "cuda":
        raise CountrError("%s needs a GPU device: the HIP path has no CPU fallback" % who)
    return device


def instance(cls, device):
    """The instance of `cls` for a device, made on first use: "cuda", "cuda:0" and torch.device("cuda", 0) give the same object."""
    device = _indexed(device)
    obj = _instances.get((cls, device))
    if obj is None:
        obj = _instances[cls, device] = cls(device)
    return obj


def grow(owner, name, n, dtype, pinned=False):
    """owner.<name>, a flat tensor on owner.device with at least n elements: made with exactly n when it is absent or smaller, never
    shrunk.  pinned=True makes owner.<name>_host, its pinned twin, in the same moment.  Call it under torch.cuda.device(owner.device)."""
    import torch
    t = getattr(owner, name)
    if t is None or t.numel() < n:
        t = torch.empty(n, dtype=dtype, device=owner.device)
        setattr(owner, name, t)
        if pinned:
            setattr(owner, name + "_host", torch.empty(n, dtype=dtype).pin_memory())
    return t


def stream_handle(device):
    """The current stream of `device` as the void* a launch takes."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Guard:
    """The cross-stream guard of a wrapper whose calls download a result and wait: a call on another stream than the last one waits for
    the last one's event before it reuses the buffers.  enter() -> the current stream, after that wait; leave(stream) records the event
    and remembers the stream; `event` is what the call then synchronises on.  Nothing is recorded before the first leave, so a first
    call waits for nothing -- unless recorded=True: the constructor filled device state on the current stream, the event is recorded
    there (make the guard under torch.cuda.device(device)), and a first call from another stream waits for that."""

    def __init__(self, device, recorded=False):
        import torch
        self.device = device
        self.event = torch.cuda.Event()
        self.last = None
        if recorded:
            self.leave(torch.cuda.current_stream(device))

    def enter(self):
        import torch
        cur = torch.cuda.current_stream(self.device)
        if self.last is not None and self.last != cur:
            cur.wait_event(self.event)
        return cur

    def leave(self, cur):
        self.event.record(cur)
        self.last = cur
