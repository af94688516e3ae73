"""Fenced device buffers for the tests of "a call stays inside the bytes its size query reports".

A `Fence` is one device allocation: a front guard, the fenced bytes, a back guard.  The guards hold a fixed two-byte pattern no
kernel produces by accident; `check()` compares them on the device and names the first and last damaged byte relative to the
fenced range.  `guarded(ctx, fill)` routes every workspace request of ONE `alac_amd.Context` instance through fences for the
duration of a with-block, so that the binding hands the library a workspace of exactly the size it asked for (the size the
`*_workspace_bytes` query reported) with memory the test owns on both sides of it.

Plain module, no fixtures: tests/ is on sys.path."""
import contextlib

FRONT_GUARD = 64 << 10  # a multiple of 256: the fenced range keeps the allocation's 256-byte alignment
MIN_BACK_GUARD = 1 << 20
OFFSET_ROOM = 256       # the largest base offset a fence can be asked for
PATTERN = (0xC3, 0x5A)  # by the parity of the byte's index in the allocation


def _align_up(x, a):
    return (x + a - 1) // a * a


def _pattern(torch, device, lo, hi):
    """the guard pattern of the allocation's bytes [lo, hi)"""
    p = torch.empty(hi - lo, dtype=torch.uint8, device=device)
    p[0::2] = PATTERN[lo & 1]
    p[1::2] = PATTERN[(lo & 1) ^ 1]
    return p


class GuardDamage(AssertionError):
    pass


class Fence:
    """front guard (64 KiB + offset) | nbytes fenced | back guard (at least max(1 MiB, nbytes)), in one allocation.

    The back guard is that large so that an overrun by one more packet slot, one more row of lanes or one more group of
    whatever the fenced bytes hold still lands in memory the test owns: a failed assertion, never a fault.
    `offset` (a multiple of 8, at most 256) shifts the fenced range's base off the allocation's 256-byte grid; `back_inset`
    begins the back guard that many bytes INSIDE the fenced range (only the detector's own test wants that); `raw` re-uses an
    earlier fence's allocation and leaves the fenced bytes as they are (real leftovers), where it is large enough."""

    def __init__(self, torch, device, nbytes, fill, offset=0, back_inset=0, raw=None, what="workspace"):
        nbytes, offset, back_inset = int(nbytes), int(offset), int(back_inset)
        assert nbytes >= 0 and 0 <= offset <= OFFSET_ROOM and offset % 8 == 0 and 0 <= back_inset <= nbytes
        self.torch, self.what, self.nbytes, self.offset, self.fill = torch, what, nbytes, offset, fill
        self.start = FRONT_GUARD + offset
        self.guard_at = self.start + nbytes - back_inset
        need = FRONT_GUARD + OFFSET_ROOM + _align_up(nbytes, 256) + max(MIN_BACK_GUARD, nbytes)
        self.reused = raw is not None and raw.numel() >= need
        if self.reused:
            self.raw = raw
            raw[:self.start] = _pattern(torch, device, 0, self.start)
            raw[self.guard_at:] = _pattern(torch, device, self.guard_at, raw.numel())
        else:
            self.raw = _pattern(torch, device, 0, need)
            self.raw[self.start:self.guard_at] = fill
        assert self.raw.data_ptr() % 256 == 0
        self.view = self.raw[self.start:self.start + nbytes]
        assert self.view.numel() == nbytes and self.view.data_ptr() == self.raw.data_ptr() + self.start
        self.checked = False

    def damage(self):
        """None, or a description of the damaged guard bytes.  The caller has synchronized."""
        t, dev, msgs = self.torch, self.raw.device, []
        end = self.start + self.nbytes
        for name, lo, hi, origin in (("front", 0, self.start, self.start), ("back", self.guard_at, self.raw.numel(), end)):
            ne = self.raw[lo:hi] != _pattern(t, dev, lo, hi)
            if bool(ne.any()):
                idx = ne.nonzero().flatten()
                first, last, count = int(idx[0]) + lo - origin, int(idx[-1]) + lo - origin, int(idx.numel())
                rel = "the %s's start" % self.what if name == "front" else "the %s's end" % self.what
                msgs.append("%s guard damaged: %d bytes, first at %+d, last at %+d relative to %s"
                            % (name, count, first, last, rel))
        if not msgs:
            return None
        return "%s of %d bytes (the size reported) at base offset %d: %s" % (self.what, self.nbytes, self.offset, "; ".join(msgs))

    def check(self):
        self.torch.cuda.synchronize()
        self.checked = True
        d = self.damage()
        if d:
            raise GuardDamage(d)

    def contents(self):
        """the fenced bytes in front of the back guard, on the host"""
        return self.raw[self.start:self.guard_at].cpu().numpy()


class Guard:
    """what guarded() yields: the fences of the block's workspace requests, oldest first"""

    def __init__(self, ctx):
        self.ctx, self.allocs = ctx, []

    def check(self):
        """after the calls: synchronizes the context, then compares every guard"""
        self.ctx.synchronize()
        assert self.allocs, "no workspace was requested inside the guarded block"
        for f in self.allocs:
            f.check()


@contextlib.contextmanager
def guarded(ctx, fill, offset=0, back_inset=0, stale=False, shrink=0):
    """Replace `ctx._workspace` on this one Context instance: every request for nbytes gets a fresh Fence whose fenced bytes
    hold `fill`, and the binding passes the view's numel() — exactly nbytes — to the library.  stale=True: a request re-uses
    the previous request's allocation, contents and all, where it fits (check() must have run on it first).  shrink=k: the
    fence, and so the size the library is told, is k bytes SHORTER than asked (the "reported size - 1" refusals).  The
    instance is restored on the way out."""
    g = Guard(ctx)
    had = "_workspace" in ctx.__dict__
    old = ctx.__dict__.get("_workspace")

    def request(nbytes):
        raw = None
        if stale and g.allocs:
            assert g.allocs[-1].checked, "check() the guards before the allocation is re-used"
            raw = g.allocs[-1].raw
        f = Fence(ctx.torch, ctx.device, int(nbytes) - shrink, fill, offset=offset, back_inset=back_inset, raw=raw)
        f.asked = int(nbytes)
        g.allocs.append(f)
        return f.view

    ctx._workspace = request
    try:
        yield g
    finally:
        if had:
            ctx._workspace = old
        else:
            del ctx.__dict__["_workspace"]
