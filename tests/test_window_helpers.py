"""The one copy of the window tests' destination checks (qb3_window_dev.py: check_destination, Layout.check) on hand-made CPU tensors:
a buffer that holds the right crops passes, and every single wrong byte -- in a payload, in front of the first window, in a wide row's
slack, between two windows, at the buffer's end -- fails.  No library call, no device."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qb3_window_dev as D  # noqa: E402

WD, HT = 20, 12
RECTS = [(0, 0, 5, 3), (7, 2, 6, 4), (13, 8, 7, 4)]
RULES = (("u8", 3, 1), ("cf8", 3, 1), ("u16", 4, 2), ("unit", 4, 2))


def raster_rows(pix):
    """a WD x HT raster as rows of bytes, none of them the sentinel"""
    import torch
    return (torch.arange(HT * WD * pix) % 128).to(torch.uint8).reshape(HT, WD * pix)


def place(buf, off, sbytes, rect, pix, rows):
    x0, y0, w, h = rect
    buf[off:off + h * sbytes].view(h, sbytes)[:, :w * pix] = rows[y0:y0 + h, x0 * pix:(x0 + w) * pix]


def flipped(buf, at):
    out = buf.clone()
    out[at] ^= 1
    return out


@pytest.mark.parametrize("rule,pix,tsz", RULES)
def test_layout_check_finds_every_wrong_byte(rule, pix, tsz):
    import torch
    rows = raster_rows(pix)
    lay = D.Layout(RECTS, pix, tsz, rule)
    good = torch.full((lay.size,), D.SENTINEL, dtype=torch.uint8)
    for r, off, sb in zip(RECTS, lay.offs, lay.sbytes):
        place(good, off, sb, r, pix, rows)
    lay.check(good, rows)
    (_, _, w1, h1), off1, sb1 = RECTS[1], lay.offs[1], lay.sbytes[1]
    assert sb1 > w1 * pix and lay.strides()[0] == 0 and lay.strides()[1] == sb1 // tsz      # window 0 tight, window 1 wide
    behind1 = off1 + h1 * sb1
    assert behind1 < lay.offs[2] and lay.offs[0] >= 1
    with pytest.raises(AssertionError, match=r"window 0 \(0, 0, 5, 3\): 1 bytes differ, the first at row 0 byte 0"):
        lay.check(flipped(good, lay.offs[0]), rows)
    with pytest.raises(AssertionError, match="window 1 .*: 1 bytes differ, the first at row %d byte %d" % (h1 - 1, w1 * pix - 1)):
        lay.check(flipped(good, off1 + (h1 - 1) * sb1 + w1 * pix - 1), rows)
    for what, at in (("in front of the first window", lay.offs[0] - 1), ("a wide row's slack", off1 + w1 * pix),
                     ("between two windows", behind1), ("the buffer's last byte", lay.size - 1)):
        with pytest.raises(AssertionError, match="outside"):
            lay.check(flipped(good, at), rows)
            pytest.fail("a wrong byte passed: " + what)
    # skip: window 1's payload is not compared, a byte written behind it is still found
    wrong = flipped(good, off1 + 2)
    with pytest.raises(AssertionError, match="differ"):
        lay.check(wrong, rows)
    lay.check(wrong, rows, skip=(1,))
    with pytest.raises(AssertionError, match="outside"):
        lay.check(flipped(wrong, behind1), rows, skip=(1,))
    lay.check(good, rows)                                                   # (check works on a copy)


@pytest.mark.parametrize("rule,pix,tsz", RULES)
def test_check_destination_finds_every_wrong_byte(rule, pix, tsz):
    import torch
    rows = raster_rows(pix)
    rect = x0, y0, w, h = RECTS[1]
    addr, extra = (3, 5) if rule == "u8" else D.destination(rule, 1, tsz)     # (the 8-bit tests hand in both)
    assert extra > 0 and addr >= 1
    sbytes = w * pix + extra * tsz
    good = torch.full((addr + (h + 1) * sbytes + 64,), D.SENTINEL, dtype=torch.uint8)
    place(good, addr, sbytes, rect, pix, rows)
    D.check_destination(good.clone(), addr, sbytes, rect, pix, rows, "w")
    with pytest.raises(AssertionError, match="w: 1 bytes differ, the first at row 2 byte 1"):
        D.check_destination(flipped(good, addr + 2 * sbytes + 1), addr, sbytes, rect, pix, rows, "w")
    for what, at in (("in front of the window", addr - 1), ("a wide row's slack", addr + w * pix), ("behind the last row", addr + h * sbytes),
                     ("the buffer's last byte", len(good) - 1)):
        with pytest.raises(AssertionError, match="w: bytes outside"):
            D.check_destination(flipped(good, at), addr, sbytes, rect, pix, rows, "w")
            pytest.fail("a wrong byte passed: " + what)
    # want_rows None (a call expected to fail): the payload is not compared, the sentinels are
    D.check_destination(flipped(good, addr), addr, sbytes, rect, pix, None, "w")
    with pytest.raises(AssertionError, match="outside"):
        D.check_destination(flipped(good, addr - 1), addr, sbytes, rect, pix, None, "w")
