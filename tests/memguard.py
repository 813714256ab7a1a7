"""Guard bands, poisoned buffers and input snapshots: the one way this suite can see a kernel that writes outside its outputs or its workspace,
reads what it never wrote, or writes an input (no GPU sanitizer, no debugger).  A plain helper module, like helpers.py.

    guarded(shape, dtype, device, poison)   one uint8 buffer [front guard 0xA5 | payload, poisoned | back guard 0xA5] -> the payload as a tensor
    Session / patched(mp, poison, ...)      for one test: cspn_amd.functional._workspace and the NAME torch inside cspn_amd.functional and
                                            cspn_amd.train_utils are replaced, so every workspace, output and history buffer the front-end
                                            allocates is guarded and poisoned; Session.check() looks at every band
    Arena                                   one workspace buffer for a whole sequence of calls, never refilled (the 'stale' mode)
    snapshot(*tensors).assert_unchanged()   the inputs, bitwise
    same_bits(a, b)                         bitwise equality with NaNs canonicalised

No global attribute of torch is touched; the patches are undone by the monkeypatch fixture (or the ExitStack) they were made through."""
import torch

GUARD_BYTE = 0xA5
FRONT_GUARD = 64 * 1024          # bytes, a multiple of 256: the payload keeps the 256-byte alignment the ABI asks of a workspace
MIN_BACK_GUARD = 64 * 1024
POISONS = ("zero", "ones", "big", "stale")
_BIG = 0x7F7FFFFF                # the largest finite float32: survives a multiplication by zero as zero, but not an addition
_BIG_BYTES = (0xFF, 0xFF, 0x7F, 0x7F)   # little endian


def _round256(n):
    return (int(n) + 255) // 256 * 256


def back_guard_bytes(plane_bytes=0):
    """at least twice the largest single plane of the case (a miscounted number of planes in a size query must land inside the band), never
    less than 64 KiB, a multiple of 256"""
    return max(MIN_BACK_GUARD, _round256(2 * int(plane_bytes)))


def poison_(payload, poison):
    """fills a uint8 view in place; 'stale' leaves it as it is"""
    if poison == "zero":
        payload.zero_()
    elif poison == "ones":
        payload.fill_(0xFF)
    elif poison == "big":
        n4 = payload.numel() // 4 * 4
        if n4:
            payload[:n4].view(torch.int32).fill_(_BIG)
        for i in range(n4, payload.numel()):
            payload[i] = _BIG_BYTES[i - n4]
    elif poison != "stale":
        raise ValueError("poison must be one of %s, got %r" % (POISONS, poison))


class Guard(object):
    """the record of one guarded region: buf[off : off + nbytes] is the payload, buf[:off] and buf[off + nbytes : end] the bands"""

    def __init__(self, buf, off, nbytes, end, name):
        self.buf, self.off, self.nbytes, self.end, self.name = buf, off, nbytes, end, name

    def lay(self):
        self.buf[:self.off].fill_(GUARD_BYTE)
        self.buf[self.off + self.nbytes:self.end].fill_(GUARD_BYTE)

    def payload(self):
        return self.buf[self.off:self.off + self.nbytes]

    def damage(self):
        """-> None, or (first, last) changed byte offset relative to the payload's first byte (negative: in the front band)"""
        if self.buf.is_cuda:
            torch.cuda.synchronize(self.buf.device)
        offsets = []
        for band, base in ((self.buf[:self.off], -self.off), (self.buf[self.off + self.nbytes:self.end], self.nbytes)):
            bad = (band != GUARD_BYTE).nonzero()
            if bad.numel():
                offsets += [base + int(bad[0]), base + int(bad[-1])]
        return (min(offsets), max(offsets)) if offsets else None

    def check(self):
        d = self.damage()
        assert d is None, ("%s: guard band overwritten: first changed byte at offset %d, last at %d, relative to a payload of %d bytes (negative: in "
                           "front of it; >= %d: behind it)" % (self.name, d[0], d[1], self.nbytes, self.nbytes))


def guarded(shape, dtype, device, poison, plane_bytes=0, name="tensor", registry=None):
    """one uint8 buffer; -> a contiguous tensor of shape / dtype inside it: 64 KiB of 0xA5 in front, back_guard_bytes(plane_bytes) of 0xA5 right
    behind its last byte (not rounded up), the payload filled with `poison`.  Its Guard is the tensor's attribute _memguard (and is appended to
    registry)"""
    shape = tuple(int(s) for s in shape)
    numel = 1
    for s in shape:
        numel *= s
    itemsize = torch.empty((), dtype=dtype).element_size()
    nbytes = numel * itemsize
    back = back_guard_bytes(plane_bytes)
    buf = torch.empty(FRONT_GUARD + _round256(nbytes) + back, dtype=torch.uint8, device=device)
    if buf.is_cuda:
        assert buf.data_ptr() % 256 == 0
    g = Guard(buf, FRONT_GUARD, nbytes, buf.numel(), name)
    g.lay()
    poison_(g.payload(), "ones" if poison == "stale" else poison)   # (a fresh buffer has nothing stale in it: NaNs, as the arena's first fill)
    t = g.payload().view(dtype).view(shape)
    assert t.is_contiguous() and (not buf.is_cuda or t.data_ptr() % 256 == 0)
    t._memguard = g
    if registry is not None:
        registry.append(g)
    return t


class Arena(object):
    """one workspace buffer for a sequence of calls, filled once (0xFF) and never again: every call gets the same first byte and finds what the
    calls before it left.  take(nbytes) lays the back guard right behind THIS call's byte count (after checking the previous call's)"""

    def __init__(self, max_bytes, device, plane_bytes=0):
        self.back = back_guard_bytes(plane_bytes)
        self.capacity = max(int(max_bytes), 1)
        self.buf = torch.empty(FRONT_GUARD + _round256(self.capacity) + self.back, dtype=torch.uint8, device=device)
        self.buf.fill_(0xFF)
        self.buf[:FRONT_GUARD].fill_(GUARD_BYTE)
        self.current = None
        self.taken = 0

    def take(self, nbytes):
        nbytes = max(int(nbytes), 1)
        assert nbytes <= self.capacity, "arena of %d bytes asked for %d" % (self.capacity, nbytes)
        self.check()
        self.current = Guard(self.buf, FRONT_GUARD, nbytes, FRONT_GUARD + nbytes + self.back, "arena workspace (call %d)" % self.taken)
        self.buf[FRONT_GUARD + nbytes:self.current.end].fill_(GUARD_BYTE)
        self.taken += 1
        return self.current.payload()

    def check(self):
        if self.current is not None:
            self.current.check()


class _TorchProxy(object):
    """what the name `torch` means inside the patched modules: the real torch, but for empty and empty_like on the session's device type"""

    def __init__(self, session):
        object.__setattr__(self, "_session", session)

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, **kw):
        s = self._session
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        device = torch.device(kw["device"]) if kw.get("device") is not None else torch.device("cpu")
        if device.type != s.device_type:
            return torch.empty(*size, **kw)
        return s.alloc(size, kw.get("dtype") or torch.get_default_dtype(), device, "torch.empty%s" % (tuple(size),))

    def empty_like(self, t, **kw):
        s = self._session
        device = torch.device(kw["device"]) if kw.get("device") is not None else t.device
        if device.type != s.device_type:
            return torch.empty_like(t, **kw)
        return s.alloc(tuple(t.shape), kw.get("dtype") or t.dtype, device, "torch.empty_like%s" % (tuple(t.shape),))


class Session(object):
    """the guarded allocations of one test.  poison: what outputs, history buffers and (without an arena) workspaces hold before the call"""

    def __init__(self, poison, device_type="cuda", plane_bytes=0, arena=None):
        if poison not in POISONS:
            raise ValueError("poison must be one of %s, got %r" % (POISONS, poison))
        self.poison, self.device_type, self.plane_bytes, self.arena = poison, device_type, plane_bytes, arena
        self.guards = []
        self.workspaces = []     # (tensor, bytes asked for), in call order
        self.torch = _TorchProxy(self)

    def alloc(self, shape, dtype, device, name):
        numel = 1
        for s in shape:
            numel *= int(s)
        if numel == 0:
            return torch.empty(tuple(shape), dtype=dtype, device=device)
        return guarded(shape, dtype, device, self.poison, self.plane_bytes, name, self.guards)

    def workspace(self, nbytes, device):
        """the replacement of cspn_amd.functional._workspace: ends exactly at the byte count the size query returned"""
        n = max(int(nbytes), 1)
        if self.arena is not None:
            ws = self.arena.take(n)
        else:
            ws = guarded((n,), torch.uint8, device, self.poison, self.plane_bytes, "workspace of %d bytes" % n, self.guards)
        self.workspaces.append((ws, int(nbytes)))
        return ws

    def check(self):
        assert self.guards or self.workspaces, "nothing was allocated through the patch: the call never reached the patched modules"
        for g in self.guards:
            g.check()
        if self.arena is not None:
            self.arena.check()


def _setattr(mp, obj, name, value):
    if hasattr(mp, "setattr"):           # pytest's monkeypatch fixture
        mp.setattr(obj, name, value)
    else:                                # a contextlib.ExitStack
        old = getattr(obj, name)
        setattr(obj, name, value)
        mp.callback(setattr, obj, name, old)


def patched(mp, poison, arena=None, device_type="cuda", plane_bytes=0, modules=None):
    """mp: the monkeypatch fixture or a contextlib.ExitStack, which undoes the patches.  modules: the namespaces whose `torch` (and, the first one's,
    `_workspace`) are replaced; default cspn_amd.functional and cspn_amd.train_utils (cspn_amd.cspn allocates nothing itself).  -> the Session"""
    if modules is None:
        from cspn_amd import functional, train_utils
        modules = (functional, train_utils)
    s = Session(poison, device_type, plane_bytes, arena)
    _setattr(mp, modules[0], "_workspace", s.workspace)
    for m in modules:
        _setattr(mp, m, "torch", s.torch)
    return s


def _bits(t):
    """a float tensor's bits with every NaN made the same one; other dtypes as they are"""
    if t.is_floating_point():
        t = torch.where(t != t, torch.full_like(t, float("nan")), t)
        return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


class Snapshot(object):
    def __init__(self, tensors):
        self.live = [t for t in tensors if isinstance(t, torch.Tensor)]
        self.kept = [t.detach().clone() for t in self.live]

    def assert_unchanged(self):
        for i, (t, k) in enumerate(zip(self.live, self.kept)):
            if t.is_cuda:
                torch.cuda.synchronize(t.device)
            if not same_bits(t.detach(), k):
                bad = (_bits(t.detach()) != _bits(k)).flatten().nonzero()
                raise AssertionError("input %d of shape %s was modified: %d elements, the first at flat index %d"
                                     % (i, tuple(t.shape), bad.numel(), int(bad[0])))


def snapshot(*tensors):
    return Snapshot(tensors)


def assert_same_outputs(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, r) in enumerate(zip(got, want)):
        if a is None or r is None:
            assert a is None and r is None, "%s: output %d is None on one side only" % (what, i)
            continue
        if not same_bits(a.detach(), r.detach()):
            d = (_bits(a.detach()) != _bits(r.detach())).flatten().nonzero() if a.shape == r.shape and a.dtype == r.dtype else None
            raise AssertionError("%s: output %d differs from the clean run%s" % (
                what, i, "" if d is None else ": %d of %d elements, the first at flat index %d" % (d.numel(), a.numel(), int(d[0]))))


def run_guarded(mp, poison, call, inputs, device_type="cuda", plane_bytes=0, arena=None, modules=None):
    """one call under the patch: -> (outputs, session) after checking every guard band and that no input changed.  mp: an ExitStack (closed by the
    caller) or monkeypatch"""
    snap = snapshot(*inputs)
    s = patched(mp, poison, arena, device_type, plane_bytes, modules)
    outs = call(*inputs)
    s.check()
    snap.assert_unchanged()
    return outs, s
