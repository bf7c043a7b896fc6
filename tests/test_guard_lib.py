"""Host-only checks of tests/guard_lib.py: the region bookkeeping and the comparison on numpy arrays (no device), and the
packed row-byte formulas the footprint tests declare, pinned against the header and the dispatch code."""
import os
import re
import subprocess

import numpy as np
import pytest

import guard_lib as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def three_planes():
    L = G.Layout()
    a = L.plane(10, 30, np.int16, stride=64, name="a")                 # row 60 bytes, 4 bytes of padding
    b = L.plane(7, 13, np.uint8, stride=13, align=64, skew=16, name="b")   # no padding, 16 but not 64 aligned
    c = L.plane(5, 9, np.int32, stride=37 * 4 + 3, align=256, skew=1, name="c", footprint=None)   # an input
    return L, a, b, c


def test_layout_guards_and_alignment():
    L, a, b, c = three_planes()
    assert a.offset >= G.GUARD_MIN and a.offset % 256 == 0
    assert b.offset - (a.offset + a.extent) >= G.GUARD_MIN and b.offset % 64 == 16
    assert c.offset - (b.offset + b.extent) >= max(G.GUARD_MIN, 2 * c.stride) and c.offset % 256 == 1
    assert L.nbytes - (c.offset + c.extent) >= G.GUARD_MIN and L.nbytes % G.CHUNK == 0
    big = G.Layout().plane(4, 4000, np.int16)
    assert big.offset >= 2 * big.stride


def test_extra_gap_between_regions():
    L = G.Layout(gap=1000)
    a = L.plane(3, 5, np.uint8, align=1)
    b = L.plane(3, 5, np.uint8, align=1)
    assert a.offset == G.GUARD_MIN + 1000 and b.offset - (a.offset + a.extent) == G.GUARD_MIN + 1000


def test_untouched_block_passes():
    L, a, b, c = three_planes()
    before = G.canary(L.nbytes, 3)
    assert G.find_changes(L, before, before.copy(), {a: a.payload(before), c: c.payload(before)}) == ([], [])


def test_writes_inside_the_footprint_are_allowed():
    L, a, b, c = three_planes()
    before = G.canary(L.nbytes, 3)
    after = before.copy()
    after[a.offset + 9 * a.stride + 59] ^= 0xff                      # last byte of a's last row
    after[b.offset:b.offset + b.extent] ^= 1                         # every byte of b
    assert G.find_changes(L, before, after) == ([], [])


@pytest.mark.parametrize("where,plane,row,col", [
    ("lead", "a", -1, 64 - 5),            # 5 bytes in front of a
    ("padding", "a", 3, 61),              # row 3's padding
    ("row after", "a", 10, 0),            # one row too many
    ("gap", "b", 7, 2),                   # in the gap after b (rows of 13 bytes)
    ("input", "c", 2, 8),                 # inside an input's rectangle
    ("tail", "c", 6, 1),                  # in the tail guard
])
def test_stray_bytes_are_reported_where_they_are(where, plane, row, col):
    L, a, b, c = three_planes()
    s = {"a": a, "b": b, "c": c}[plane]
    before = G.canary(L.nbytes, 5)
    after = before.copy()
    off = s.offset + row * s.stride + col
    after[off] ^= 0x41
    mism, strays = G.find_changes(L, before, after, {a: a.payload(before)})
    assert mism == [] and len(strays) == 1, (where, strays)
    assert strays[0].startswith("%s: 1 stray bytes, first at (row,col)=(%d,%d)" % (plane, row, col)), strays
    assert "canary 0x%02x, found 0x%02x" % (before[off], after[off]) in strays[0]


def test_every_stray_region_is_named_and_counted():
    L, a, b, c = three_planes()
    before = G.canary(L.nbytes, 7)
    after = before.copy()
    after[a.offset - 1] ^= 1
    after[b.offset + b.extent: b.offset + b.extent + 3] ^= 1
    mism, strays = G.find_changes(L, before, after)
    assert mism == [] and len(strays) == 2
    assert strays[0].startswith("a: 1 stray bytes") and strays[1].startswith("b: 3 stray bytes, first at (row,col)=(7,0)")
    with pytest.raises(AssertionError, match="STRAY WRITE -- b: 3"):
        G.report(mism, strays)


def test_a_payload_mismatch_is_not_a_stray_write():
    L, a, b, c = three_planes()
    before = G.canary(L.nbytes, 9)
    after = before.copy()
    off = a.offset + 4 * a.stride + 2 * 7                          # a[4, 7]
    after[off] ^= 0x10
    want = a.payload(before)
    mism, strays = G.find_changes(L, before, after, {a: want})
    assert strays == [] and len(mism) == 1 and mism[0].startswith("a: 1 payload mismatches, first at (y,x)=(4,7)"), mism


def test_rectangle_lists_and_byte_ranges():
    L = G.Layout()
    d = L.plane(8, 8, np.int16, stride=32, footprint=[(0, 64, 4, 4), (16 + 2, 64, 6, 2)], name="d")
    h = L.span(1000, align=128, footprint=("bytes", 1000), name="h", stride=512)
    assert h.offset % 128 == 0 and h.offset - (d.offset + d.extent) >= G.GUARD_MIN
    before = G.canary(L.nbytes, 11)
    ok = before.copy()
    for (o, st, rb, rows) in d.footprint:
        for r in range(rows):
            ok[d.offset + o + r * st: d.offset + o + r * st + rb] ^= 1
    ok[h.offset:h.offset + 1000] ^= 1
    assert G.find_changes(L, before, ok) == ([], [])
    bad = before.copy()
    bad[d.offset + 32] ^= 1                           # row 1: between the codeblocks' rows (dst_stride 64)
    bad[h.offset + 1000] ^= 1                         # one past the half-pel image
    _, strays = G.find_changes(L, before, bad)
    assert [s.split(",")[0] for s in strays] == ["d: 1 stray bytes", "h: 1 stray bytes"], strays
    assert "(row,col)=(1,0)" in strays[0]


def test_packed_row_bytes():
    F = G.packed_row_bytes
    for w in (1, 2, 5, 6, 7, 12, 13, 1919, 1920):
        assert F(0x106, w) == 16 * -(-w // 6)             # v210
        assert F(0x105, w) == 8 * (w // 2)                # v216: an odd width drops its last pixel
        assert F(0x100, w) == F(0x101, w) == 4 * (w // 2)  # YUYV / UYVY
        assert F(0x102, w) == F(0x103, w) == 4 * w        # AYUV / ARGB
        assert F(0x107, w) == 8 * w                       # AY64
    assert (F(0x105, 7), F(0x106, 7), F(0x100, 7)) == (24, 32, 12)


def test_packed_row_bytes_match_the_header_and_the_dispatch(tmp_path):
    """The row-byte expression of plane_frameops.cpp, compiled as it stands against the header's format values, gives
    packed_row_bytes for every packed format and a range of widths."""
    src = open(os.path.join(ROOT, "schroedinger_amd", "csrc", "plane_frameops.cpp")).read()
    expr = re.search(r"const int row_bytes = (.*?);", src, re.S).group(1)
    cases = [(1, 0, 0x106), (0, 2, 0x105), (0, 2, 0x103), (0, 2, 0x107), (0, 0, 0x100), (0, 0, 0x101), (0, 0, 0x102)]
    widths = list(range(1, 26)) + [1919, 1920, 3841]
    prog = tmp_path / "row_bytes.c"
    prog.write_text("""#include <stdio.h>
#include "schro_hip.h"
static int div_up (int a, int b) { return (a + b - 1) / b; }
struct P { int width, format; };
static int row_bytes (int v210_bpp, int wide_bpp, int format, int width)
{
  struct P pl = { width, format };
  return %s;
}
int main (void)
{
  static const int cases[][3] = { %s };
  static const int widths[] = { %s };
  for (unsigned c = 0; c < sizeof cases / sizeof cases[0]; c++)
    for (unsigned w = 0; w < sizeof widths / sizeof widths[0]; w++)
      printf ("%%d %%d %%d\\n", cases[c][2], widths[w], row_bytes (cases[c][0], cases[c][1], cases[c][2], widths[w]));
  return 0;
}
""" % (expr, ", ".join("{%d, %d, %d}" % c for c in cases), ", ".join(map(str, widths))))
    exe = tmp_path / "row_bytes"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    rows = [tuple(map(int, ln.split())) for ln in subprocess.run([str(exe)], check=True, capture_output=True,
                                                                 text=True).stdout.split("\n") if ln]
    assert len(rows) == len(cases) * len(widths)
    for fmt, w, n in rows:
        assert n == G.packed_row_bytes(fmt, w), (hex(fmt), w, n)
    hdr = open(os.path.join(ROOT, "include", "schro_hip.h")).read()
    assert "YUYV / UYVY write width / 2 four-byte groups per row, AYUV width." in hdr
    assert "v210: 16 bytes per 6 pixels" in hdr
