"""The checker checked: tests/_arena.py on CPU tensors.  Every stray access is done HERE with a plain tensor write -- no library
call is involved -- and the arena must name the region, the side, the offsets and the byte count."""
import numpy as np
import pytest
import torch

from _arena import GUARD_MAX, GUARD_MIN, SENTINEL_BYTE, SENTINEL_WORD, Arena, ArenaViolation, guard_bytes


def _arena():
    rng = np.random.default_rng(7)
    a = Arena("cpu")
    a.add("P", "in", data=rng.normal(size=1031).astype(np.float32), residue=4, row_bytes=1031 * 4)
    a.add("s", "in", data=rng.uniform(1, 2, size=5).astype(np.float32))
    a.add("out", "out", nbytes=1031 * 4, residue=4, row_bytes=1031 * 4)
    a.add("q8", "out", nbytes=1031)                                   # byte-exact: 1031 is no multiple of 4
    a.add("ws", "ws", nbytes=4096)
    a.add("bins", "some", nbytes=64)
    a.add("m", "inout", data=np.zeros(5, np.float32))
    a.add("wide", "out", nbytes=16, row_bytes=3 << 20)                 # two rows above the cap
    return a.build()


def _fill_outputs(a):
    for name in ("out", "q8", "wide"):
        a.bytes(name).fill_(1)


def test_sentinel_values():
    w = np.array([SENTINEL_WORD, SENTINEL_WORD], np.uint32)
    assert 3.39e38 < w.view(np.float32)[0] < 3.40e38 and np.isfinite(w.view(np.float32)[0])
    assert 1.3e306 < w.view(np.float64)[0] < 1.5e306
    assert int(w[0]) == 2139062143
    assert bytes([SENTINEL_BYTE] * 4) == w[:1].tobytes()


def test_layout_residues_sizes_guards_and_no_overlap():
    a = _arena()
    spans = []
    for name in a.names():
        r = a.region(name)
        lo, hi = a.span(name)
        assert a.ptr(name) % 16 == r.residue, name
        assert hi - lo == r.nbytes == a.nbytes(name), name
        spans.append((lo, hi, r.guard, name))
    assert a.ptr("ws") % 16 == 0 and a.ptr("P") % 16 == 4 and a.ptr("out") % 16 == 4
    assert a.nbytes("q8") == 1031
    spans.sort()
    assert spans[0][0] >= spans[0][2], "guard in front of the first region"
    assert a.buf.numel() - spans[-1][1] >= spans[-1][2], "guard behind the last region"
    for (lo0, hi0, g0, n0), (lo1, hi1, g1, n1) in zip(spans, spans[1:]):
        assert lo1 - hi0 >= max(g0, g1), f"guard between {n0} and {n1}"
    assert guard_bytes(0) == GUARD_MIN and guard_bytes(1031 * 4) == GUARD_MIN
    assert guard_bytes(40000) == 80000 and guard_bytes(3 << 20) == GUARD_MAX
    assert a.region("wide").guard == GUARD_MAX
    # the uploads are where the pointers say, everything else is sentinel
    assert np.array_equal(a.numpy("s", np.float32), a.region("s").data)
    covered = torch.zeros(a.buf.numel(), dtype=torch.bool)
    for lo, hi, _, _ in spans:
        assert not covered[lo:hi].any()
        covered[lo:hi] = True
    assert bool((a.buf[~covered] == SENTINEL_BYTE).all())
    assert bool((a.view("out", torch.int32) == SENTINEL_WORD).all())


def test_clean_run_passes():
    a = _arena()
    _fill_outputs(a)
    a.fill("ws", 0xFF)                                                 # scratch and partly filled outputs may hold anything
    a.view("bins", torch.int32)[3] = 9
    a.view("m", torch.float32)[0] = 1.5                                # in-place state may change
    assert a.violations() == []
    a.check("clean")


def _single(a):
    with pytest.raises(ArenaViolation) as e:
        a.check("case X")
    assert len(e.value.findings) == 1, e.value.findings
    assert "case X" in str(e.value)
    return e.value.findings[0], str(e.value)


@pytest.mark.parametrize("name", ["P", "out", "q8", "ws", "m"])
def test_first_guard_byte_before_a_region(name):
    a = _arena()
    _fill_outputs(a)
    lo, _ = a.span(name)
    a.buf[lo - 1] = 0
    f, msg = _single(a)
    assert f == dict(region=name, where="before", first=-1, last=-1, count=1)
    assert f"{name}: before, 1 bytes, offsets -1..-1" in msg


@pytest.mark.parametrize("name", ["P", "out", "q8", "ws", "m", "wide"])
def test_last_guard_byte_after_a_region(name):
    """The far end of the guard behind a region: for the last region that is the arena's last byte, otherwise the last byte of
    the first half of the gap (the second half belongs to the next region's front)."""
    a = _arena()
    _fill_outputs(a)
    _, hi = a.span(name)
    order = sorted(a.names(), key=lambda n: a.span(n)[0])
    i = order.index(name)
    end = a.buf.numel() if i + 1 == len(order) else (hi + a.span(order[i + 1])[0]) // 2
    assert end - hi >= a.region(name).guard // 2
    a.buf[end - 1] ^= 0x01                                             # one bit of one byte
    f, _ = _single(a)
    assert f == dict(region=name, where="after", first=end - 1 - hi, last=end - 1 - hi, count=1)
    # and the very first byte behind the region
    b = _arena()
    _fill_outputs(b)
    b.buf[b.span(name)[1]] = 0
    f, _ = _single(b)
    assert f == dict(region=name, where="after", first=0, last=0, count=1)


def test_store_one_element_past_an_output_is_four_bytes_after_it():
    a = _arena()
    _fill_outputs(a)
    _, hi = a.span("out")
    a.buf[hi:hi + 4] = torch.tensor([0, 0, 128, 63], dtype=torch.uint8)
    f, _ = _single(a)
    assert f == dict(region="out", where="after", first=0, last=3, count=4)


def test_changed_input_element():
    a = _arena()
    _fill_outputs(a)
    v = a.view("P", torch.float32)
    v[700] = -v[700]                                                   # the sign bit: byte 3 of element 700
    f, msg = _single(a)
    assert f == dict(region="P", where="input changed", first=700 * 4 + 3, last=700 * 4 + 3, count=1)
    assert "P: input changed" in msg


def test_unwritten_output_element():
    a = _arena()
    _fill_outputs(a)
    a.view("out", torch.int32)[1030] = SENTINEL_WORD                   # the last element left as it was
    f, msg = _single(a)
    assert f == dict(region="out", where="output unwritten", first=1030 * 4, last=1030 * 4 + 3, count=4)
    assert "out: output unwritten" in msg
    # a byte-sized view: whole words only -- bytes 1028..1030 of q8 are left to the comparison with the reference
    b = _arena()
    _fill_outputs(b)
    b.bytes("q8")[8:12] = SENTINEL_BYTE
    b.bytes("q8")[1028:] = SENTINEL_BYTE
    f, _ = _single(b)
    assert f == dict(region="q8", where="output unwritten", first=8, last=11, count=4)


def test_several_findings_are_all_reported():
    a = _arena()                                                       # outputs never written at all
    lo, hi = a.span("ws")
    a.buf[lo - 16:lo] = 0
    a.buf[hi + 100] = 0
    with pytest.raises(ArenaViolation) as e:
        a.check("many")
    got = {(f["region"], f["where"]): (f["first"], f["last"], f["count"]) for f in e.value.findings}
    assert got[("ws", "before")] == (-16, -1, 16)
    assert got[("ws", "after")] == (100, 100, 1)
    assert got[("out", "output unwritten")] == (0, 1031 * 4 - 1, 1031 * 4)
    assert got[("q8", "output unwritten")] == (0, 1027, 1028)
    assert got[("wide", "output unwritten")] == (0, 15, 16)
    assert len(got) == 5


def test_upload_replaces_the_pristine_copy():
    a = _arena()
    _fill_outputs(a)
    new = np.arange(5, dtype=np.float32)
    a.upload("s", new)
    a.check("second run")
    assert np.array_equal(a.numpy("s", np.float32), new)


def test_outputs_of_other_calls_must_stay_untouched():
    """check(written=[...]): only the named outputs must be full; every other "out" region must still be all sentinel."""
    a = _arena()
    a.bytes("out").fill_(1)
    a.check("one call", written=["out"])
    with pytest.raises(ArenaViolation):
        a.check("all outputs")                                        # q8 and wide were never written
    a.bytes("q8")[5] = 0
    with pytest.raises(ArenaViolation) as e:
        a.check("one call", written=["out"])
    assert e.value.findings == [dict(region="q8", where="output of another call written", first=5, last=5, count=1)]


def test_repair_restores_the_guards_only():
    a = _arena()
    _fill_outputs(a)
    lo, hi = a.span("ws")
    a.buf[lo - 3] = 0
    a.buf[hi + 9] = 0
    a.buf[0] = 1
    a.buf[-1] = 1
    inside = a.buf[lo:hi].clone().fill_(0x11)
    a.buf[lo:hi] = inside
    assert len(a.violations()) == 4
    a.repair()
    assert a.violations() == []
    assert torch.equal(a.buf[lo:hi], inside) and bool((a.bytes("out") == 1).all())
