"""A guarded arena for buffer-contract tests of the C ABI (include/lcp_hip.h).

Every buffer of one call sequence - inputs, outputs, counts, status words, the workspace - is carved from ONE `torch.uint8` tensor.
Each buffer starts on a 256-byte boundary and has a guard band of its own before it and after it (the arena therefore begins and
ends with a guard).  Guards and outputs are filled with a known byte before the call; `check()` afterwards names every guard a
kernel wrote into.  Because the arena is one allocation a modest overrun lands in a guard, where it is reported - it never leaves
allocated memory, so a misbehaving kernel fails the test instead of faulting the device.

    ar = Arena(B, device)
    ar.add("v", torch.float32, (B, nb, 3), data=v)                 # an input (const: role "in")
    ar.add("v_new", torch.float32, (B, nb, 3))                     # an output: 0xFF bytes = NaN floats / -1 ints
    ar.add("ws", torch.uint8, (nbytes,), role="ws")
    ar.build()
    snap = ar.snapshot_inputs()
    rc = lib.lcp_...(.., ar.ptr("v"), .., ar.ptr("v_new"), ar.ptr("ws"), stream)
    ar.sync(); assert ar.check() == [] and ar.inputs_unchanged(snap) == []

A single run cannot see a stray store of the fill byte itself (NaN / -1 patterns into 0xFF guards, zeros into 0x00 guards): run a
case once with each fill.  The leading guard is a fixed 4096 bytes and only the trailing one scales with the bytes per scene, so a
store far in front of a large-stride buffer (a negative scene index on the workspace, say) lands in the previous buffer's trailing
guard or payload and is reported under that neighbour's name - it still cannot leave the arena.

No GPU is needed for the arena itself (tests/test_guarded_buffers_host.py exercises it on the CPU)."""
import ctypes

import torch

ALIGN = 256
GUARD_MIN = 4096
OUT_FILL = 0xFF              # NaN as float32 / float64, -1 as int32


def _round_up(n, a=ALIGN):
    return (int(n) + a - 1) // a * a


def trailing_guard_bytes(nbytes, B):
    """max(4096, 4 x the buffer's bytes per scene), rounded up to 256: a kernel that packs four scenes into a wavefront and stores
    for three scenes that do not exist still lands inside the arena."""
    per_scene = (int(nbytes) + max(int(B), 1) - 1) // max(int(B), 1)
    return _round_up(max(GUARD_MIN, 4 * per_scene))


class _Buf:
    __slots__ = ("name", "dtype", "shape", "role", "data", "nbytes", "start", "before", "after")


class Arena:
    """`B`: scenes per buffer (it sizes the trailing guards).  `fill`: the byte guards and the workspace are prefilled with (outputs
    always get 0xFF so that an element nobody wrote stays recognisable).  `reverse`: carve the buffers in reverse order of `add`."""

    def __init__(self, B, device="cpu", fill=0xFF, reverse=False):
        self.B, self.device, self.fill, self.reverse = int(B), torch.device(device), int(fill), bool(reverse)
        self._specs, self._bufs, self.mem = [], {}, None

    def add(self, name, dtype, shape, role=None, data=None):
        """role: "in" (default with `data`), "out" (default without), "inout" (data given, the call may write it), "ws"."""
        if self.mem is not None or name in self._bufs or any(s.name == name for s in self._specs):
            raise ValueError("buffer %r: already carved" % (name,))
        b = _Buf()
        b.name, b.dtype, b.shape = name, dtype, tuple(int(s) for s in shape)
        b.role = role or ("in" if data is not None else "out")
        if b.role not in ("in", "out", "inout", "ws") or (b.role in ("in", "inout")) != (data is not None):
            raise ValueError("buffer %r: role %r %s data" % (name, b.role, "needs" if data is None else "takes no"))
        b.data = data
        n = 1
        for s in b.shape:
            n *= s
        b.nbytes = n * torch.empty(0, dtype=dtype).element_size()
        self._specs.append(b)
        return self

    def build(self):
        order = list(reversed(self._specs)) if self.reverse else list(self._specs)
        off = 0
        for b in order:
            b.before = (off, off + GUARD_MIN)
            b.start = off + GUARD_MIN
            end = b.start + b.nbytes
            off = _round_up(end) + trailing_guard_bytes(b.nbytes, self.B)
            b.after = (end, off)
        total = max(off, GUARD_MIN)
        raw = torch.empty(total + ALIGN, dtype=torch.uint8, device=self.device)
        shift = (-raw.data_ptr()) % ALIGN                      # (the allocators align to less than 256 bytes on some devices)
        self._raw, self.mem = raw, raw[shift:shift + total]
        self.mem.fill_(self.fill)
        self._guard = torch.zeros(total, dtype=torch.bool, device=self.device)
        for b in order:
            self._bufs[b.name] = b
            self._guard[b.before[0]:b.before[1]] = True
            self._guard[b.after[0]:b.after[1]] = True
            if b.role in ("in", "inout"):
                self[b.name].copy_(b.data.to(dtype=b.dtype).reshape(b.shape))
            elif b.role == "out":
                self.bytes_of(b.name).fill_(OUT_FILL)
            assert (self.mem.data_ptr() + b.start) % ALIGN == 0
        return self

    # ---- access ----
    def __contains__(self, name):
        return name in self._bufs

    def names(self, *roles):
        return [n for n, b in self._bufs.items() if not roles or b.role in roles]

    def span(self, name):
        """(start, nbytes, before, after): byte offsets into `mem` of the buffer, its size, and the (lo, hi) ranges of its two guards."""
        b = self._bufs[name]
        return b.start, b.nbytes, b.before, b.after

    def order(self):
        """Buffer names in the order of `add` (names() lists them in carving order)."""
        return [s.name for s in self._specs if s.name in self._bufs]

    def role(self, name):
        return self._bufs[name].role

    def bytes_of(self, name):
        b = self._bufs[name]
        return self.mem[b.start:b.start + b.nbytes]

    def __getitem__(self, name):
        b = self._bufs[name]
        return self.bytes_of(name).view(b.dtype).view(b.shape)

    def ptr(self, name):
        """Pointer for the C ABI (None = NULL for a name that is None or was not carved)."""
        if name is None or name not in self._bufs:
            return None
        return ctypes.c_void_p(self.mem.data_ptr() + self._bufs[name].start)

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    # ---- checks ----
    def check(self):
        """Guard bytes that no longer hold the fill: [(buffer, "before" | "after", first, last)] with byte offsets relative to
        the start of that buffer (negative in a leading guard, >= the buffer's size in a trailing one)."""
        bad = (self.mem != self.fill) & self._guard
        if not bool(bad.any()):
            return []
        out = []
        for b in self._bufs.values():
            for side, (lo, hi) in (("before", b.before), ("after", b.after)):
                idx = bad[lo:hi].nonzero()
                if idx.numel():
                    out.append((b.name, side, lo + int(idx[0]) - b.start, lo + int(idx[-1]) - b.start))
        return out

    def snapshot_inputs(self, names=None):
        """Copies of the const buffers (default: every buffer of role "in")."""
        names = self.names("in") if names is None else list(names)
        return {n: self.bytes_of(n).clone() for n in names}

    def inputs_unchanged(self, snap, exempt=()):
        """Names of snapshotted buffers that are no longer bitwise what they were, as [(name, first, last)] byte offsets.  `exempt`:
        buffers the call may legitimately write (`jrot1` of lcp_joint_jacobian_f64; a `p` that was passed as `p_out` too)."""
        out = []
        for n, old in snap.items():
            if n in exempt:
                continue
            idx = (self.bytes_of(n) != old).nonzero()
            if idx.numel():
                out.append((n, int(idx[0]), int(idx[-1])))
        return out

    def tag(self, name="ws"):
        """The layout tag a forward leaves in the workspace trailer: the first word of the last 256 bytes."""
        w = self.bytes_of(name)
        return int(w[w.numel() - 256:w.numel() - 252].cpu().view(torch.int32)[0])
