"""A poisoned arena for the memory-contract tests (tests/test_gpu_memory_contract*.py; checked itself by tests/test_arena_cpu.py).

ONE allocation per test case, every byte preset to the sentinel 0x7F (the word 0x7F7F7F7F: 3.4e38 as float32 -- finite and
huge, so it survives a max and wrecks a sum or a count where a NaN would be dropped by an fmax --, ~1.4e306 as float64,
2 139 062 143 as uint32).  Every pointer a call receives -- inputs, outputs, workspace -- is a region carved out of it:

  * a region starts at the requested residue mod 16 of its ADDRESS and has exactly the stated size, to the byte;
  * regions are separated from each other and from both ends of the arena by guards of at least GUARD_MIN bytes and at least
    two "rows" of the region (``row_bytes``: inner * 4 of a row form, G * inner * 4 of a column form), capped at GUARD_MAX: an
    access that is off by one row or one layer still lands inside the arena, where it is an ordinary store that check() sees.

check(what), after the device has been synchronised, holds the call to its contract:

  * every guard byte still holds the sentinel;
  * every region of kind "in" is bit for bit what was uploaded;
  * every region of kind "out" (an output the call must fill completely) holds no sentinel word -- an element left unwritten
    shows.  Whole 32-bit words only: the last size % 4 bytes of a byte-sized view are left to the test's comparison with the
    reference, where a single legitimate int8 127 cannot be mistaken for the poison;
  * kinds "ws" (scratch), "inout" (uploaded, changed in place) and "some" (an output that is filled only in part, bins for
    instance) are held to their guards alone; what they contain is the business of the comparison with the reference.

The gap between two regions is one stretch of sentinel; its first half is reported as "after" the region in front of it, its
second half as "before" the region behind it.  A finding names the region, the side, the first and the last offending byte as
offsets from that edge of the region (after: 0 is the first byte behind the region; before: -1 is the last byte in front of it;
inside a region: 0 is its first byte) and the number of bytes hit.  Comparisons run on the device the arena lives on; bytes are
copied to the host only to describe a failure."""
import numpy as np
import torch

SENTINEL_BYTE = 0x7F
SENTINEL_WORD = 0x7F7F7F7F
GUARD_MIN = 64 << 10
GUARD_MAX = 4 << 20
KINDS = ("in", "out", "ws", "inout", "some")


class ArenaViolation(AssertionError):
    """check() found something; ``findings`` is the list of dicts (region, where, first, last, count) behind the message."""

    def __init__(self, message, findings):
        super().__init__(message)
        self.findings = findings


class _Region:
    __slots__ = ("name", "kind", "nbytes", "residue", "guard", "data", "start", "pristine")

    def __init__(self, name, kind, nbytes, residue, guard, data):
        self.name, self.kind, self.nbytes, self.residue, self.guard, self.data = name, kind, nbytes, residue, guard, data
        self.start = None
        self.pristine = None


def guard_bytes(row_bytes=0):
    return int(min(max(GUARD_MIN, 2 * int(row_bytes)), GUARD_MAX))


class Arena:
    def __init__(self, device):
        self.device = torch.device(device)
        self._regions = {}
        self.buf = None

    # ------------------------------------------------------------------ layout
    def add(self, name, kind, nbytes=None, data=None, residue=0, row_bytes=0):
        """Declares a region.  ``data`` (a NumPy array; required for "in" and "inout", allowed for "ws") is uploaded by build()
        and fixes the size; otherwise ``nbytes`` does.  Returns ``name``."""
        assert self.buf is None, "add() after build()"
        assert kind in KINDS and name not in self._regions and residue in (0, 4, 8, 12)
        if data is not None:
            data = np.ascontiguousarray(data)
            assert nbytes is None or nbytes == data.nbytes
            nbytes = data.nbytes
        assert nbytes is not None and nbytes > 0, f"{name}: a region needs a size"
        assert data is not None or kind not in ("in", "inout"), f"{name}: an input region needs its data"
        self._regions[name] = _Region(name, kind, int(nbytes), residue, guard_bytes(row_bytes), data)
        return name

    def build(self):
        """Allocates the arena, places the regions in the order they were declared and uploads their data."""
        regs = list(self._regions.values())
        total = 16                                            # slack for the alignment of the allocation itself
        for i, r in enumerate(regs):
            total += max(r.guard, regs[i - 1].guard if i else 0) + 32 + r.nbytes
        total += regs[-1].guard + 16
        self.buf = torch.full((total,), SENTINEL_BYTE, dtype=torch.uint8, device=self.device)
        base = self.buf.data_ptr()
        cursor = 0
        for i, r in enumerate(regs):
            lo = cursor + max(r.guard, regs[i - 1].guard if i else 0)
            r.start = lo + (r.residue - (base + lo)) % 16
            cursor = r.start + r.nbytes
        assert cursor + regs[-1].guard <= total
        for r in regs:
            if r.data is not None:
                host = torch.tensor(r.data.reshape(-1).view(np.uint8))      # a copy: the caller's array may be read-only
                dev = host.to(self.device) if self.device.type != "cpu" else host.clone()
                self.bytes(r.name).copy_(dev)
                if r.kind == "in":
                    r.pristine = dev
        return self

    # ------------------------------------------------------------------ access
    def region(self, name):
        return self._regions[name]

    def names(self):
        return list(self._regions)

    def span(self, name):
        """(first byte, one past the last byte) of the region as offsets into the arena."""
        r = self._regions[name]
        return r.start, r.start + r.nbytes

    def ptr(self, name):
        return self.buf.data_ptr() + self._regions[name].start

    def nbytes(self, name):
        return self._regions[name].nbytes

    def bytes(self, name):
        a, b = self.span(name)
        return self.buf[a:b]

    def view(self, name, dtype):
        """The region as a flat tensor of ``dtype`` (a view into the arena; the size must be a whole number of elements)."""
        return self.bytes(name).view(dtype)

    def numpy(self, name, dtype):
        return self.bytes(name).cpu().numpy().view(dtype)

    def fill(self, name, byte):
        self.bytes(name).fill_(byte)

    def upload(self, name, data):
        """Replaces the contents (and, for an input, the pristine copy) of a region: the next run of the same case."""
        r = self._regions[name]
        host = torch.tensor(np.ascontiguousarray(data).reshape(-1).view(np.uint8))
        assert host.numel() == r.nbytes
        dev = host.to(self.device) if self.device.type != "cpu" else host.clone()
        self.bytes(name).copy_(dev)
        if r.kind == "in":
            r.pristine = dev

    # ------------------------------------------------------------------ the check
    def _gaps(self):
        """[(a, b, region in front or None, region behind or None)] -- every stretch of the arena outside the regions."""
        regs = sorted(self._regions.values(), key=lambda r: r.start)
        gaps, cursor, prev = [], 0, None
        for r in regs:
            gaps.append((cursor, r.start, prev, r))
            cursor, prev = r.start + r.nbytes, r
        gaps.append((cursor, self.buf.numel(), prev, None))
        return gaps

    def _describe(self, lo, hi, region, where, edge, findings, differs=None):
        """Adds the finding for the offending bytes of arena[lo:hi]; ``differs``: host bool array, default != sentinel."""
        if differs is None:
            differs = self.buf[lo:hi].cpu().numpy() != SENTINEL_BYTE
        idx = np.flatnonzero(differs)
        if idx.size:
            findings.append(dict(region=region, where=where, first=int(lo + idx[0] - edge), last=int(lo + idx[-1] - edge),
                                 count=int(idx.size)))

    def violations(self, written=None):
        """The list of findings (empty: the contract holds).  ``written``: the "out" regions this call must have filled (default:
        all of them); every other "out" region must still hold the sentinel in every byte."""
        assert self.buf is not None
        idle = set() if written is None else {n for n, r in self._regions.items() if r.kind == "out"} - set(written)
        gaps = self._gaps()
        flags = [(self.buf[a:b] != SENTINEL_BYTE).any() for a, b, _, _ in gaps]
        regs = list(self._regions.values())
        for r in regs:
            if r.kind == "in":
                flags.append((self.bytes(r.name) != r.pristine).any())
            elif r.name in idle:
                flags.append((self.bytes(r.name) != SENTINEL_BYTE).any())
            elif r.kind == "out":
                words = self.buf[r.start:r.start + (r.nbytes & ~3)]
                flags.append((words.view(torch.int32) == SENTINEL_WORD).any() if words.numel() else
                             torch.zeros((), dtype=torch.bool, device=self.device))
            else:
                flags.append(torch.zeros((), dtype=torch.bool, device=self.device))
        hit = torch.stack(flags).cpu().numpy()                 # one transfer for the whole verdict
        findings = []
        if not hit.any():
            return findings
        for (a, b, front, behind), bad in zip(gaps, hit[:len(gaps)]):
            if not bad:
                continue
            mid = b if behind is None else (a if front is None else (a + b) // 2)
            if front is not None:
                self._describe(a, mid, front.name, "after", a, findings)
            if behind is not None:
                self._describe(mid, b, behind.name, "before", b, findings)
        for r, bad in zip(regs, hit[len(gaps):]):
            if not bad:
                continue
            if r.kind == "in":
                differs = (self.bytes(r.name) != r.pristine).cpu().numpy()
                self._describe(r.start, r.start + r.nbytes, r.name, "input changed", r.start, findings, differs)
            elif r.name in idle:
                self._describe(r.start, r.start + r.nbytes, r.name, "output of another call written", r.start, findings)
            else:
                w = self.buf[r.start:r.start + (r.nbytes & ~3)].cpu().numpy().view(np.uint32) == SENTINEL_WORD
                self._describe(r.start, r.start + (r.nbytes & ~3), r.name, "output unwritten", r.start, findings, np.repeat(w, 4))
        return findings

    def repair(self):
        """Every guard byte back to the sentinel: after a reported violation the next call on the same arena is judged on its own."""
        for a, b, _, _ in self._gaps():
            self.buf[a:b] = SENTINEL_BYTE

    def check(self, what="", written=None):
        findings = self.violations(written)
        if findings:
            lines = [f"{f['region']}: {f['where']}, {f['count']} bytes, offsets {f['first']}..{f['last']}" for f in findings]
            raise ArenaViolation(f"{what}: memory contract broken -- " + "; ".join(lines), findings)
