"""Writes csrc/font_atlas.h: the 1-bit bitmap fonts the frame renderer (csrc/render.hip) draws text with.

ASCII 32..126 of DejaVu Sans Mono (labels and zone names, cap height 10 px) and DejaVu Sans Mono Bold (the HUD, cap height
17 px), rasterised with PIL and thresholded at half coverage.  Every glyph is a cell `advance` pixels wide and
`ascent + descent` rows tall; row 0 is `ascent` rows above the baseline, bit k of a row word is column k.  ascent / descent
are the ink bounds over the whole set (tight, so a label box is as tall as the text it holds).

The header is committed: building or running the library needs neither PIL nor the TTF files.  Re-run after changing a size:
    python tools/gen_font_atlas.py            # writes the header
    python tools/gen_font_atlas.py --check    # exit 1 if the committed header differs from a fresh run
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "real-time-multi-object-detection---tracking-system_amd", "csrc", "font_atlas.h")
FIRST, LAST = 32, 126
# (file name, pixel size): font 0 = labels / zone names, font 1 = HUD
FONTS = [("DejaVuSansMono.ttf", 14), ("DejaVuSansMono-Bold.ttf", 23)]
# an explicit directory first (--font-dir), then the system fonts as PIL finds them by name, then matplotlib's bundled copies
FONT_DIRS: list = []

LICENCE = """\
 * Glyph bitmaps rasterised from the DejaVu fonts (DejaVu Sans Mono, DejaVu Sans Mono Bold).
 * Copyright (c) 2003 by Bitstream, Inc. All Rights Reserved. Bitstream Vera is a trademark of Bitstream, Inc.
 * DejaVu changes are in public domain.
 *
 * Permission is hereby granted, free of charge, to any person obtaining a copy of the fonts accompanying this license ("Fonts")
 * and associated documentation files (the "Font Software"), to reproduce and distribute the Font Software, including without
 * limitation the rights to use, copy, merge, publish, distribute, and/or sell copies of the Font Software, and to permit persons
 * to whom the Font Software is furnished to do so, subject to the following conditions:
 *
 * The above copyright and trademark notices and this permission notice shall be included in all copies of one or more of the
 * Font Software typefaces.
 *
 * The Font Software may be modified, altered, or added to, and in particular the designs of glyphs or characters in the Fonts
 * may be modified and additional glyphs or characters may be added to the Fonts, only if the fonts are renamed to names not
 * containing either the words "Bitstream" or the word "Vera".
 *
 * This License becomes null and void to the extent applicable to Fonts or Font Software that has been modified and is
 * distributed under the "Bitstream Vera" names.
 *
 * The Font Software may be sold as part of a larger software package but no copy of one or more of the Font Software typefaces
 * may be sold by itself.
 *
 * THE FONT SOFTWARE IS PROVIDED "AS IS", WITHOUT WARRANTY OF ANY KIND, EXPRESS OR IMPLIED, INCLUDING BUT NOT LIMITED TO ANY
 * WARRANTIES OF MERCHANTABILITY, FITNESS FOR A PARTICULAR PURPOSE AND NONINFRINGEMENT OF COPYRIGHT, PATENT, TRADEMARK, OR OTHER
 * RIGHT. IN NO EVENT SHALL BITSTREAM OR THE GNOME FOUNDATION BE LIABLE FOR ANY CLAIM, DAMAGES OR OTHER LIABILITY, INCLUDING ANY
 * GENERAL, SPECIAL, INDIRECT, INCIDENTAL, OR CONSEQUENTIAL DAMAGES, WHETHER IN AN ACTION OF CONTRACT, TORT OR OTHERWISE, ARISING
 * FROM, OUT OF THE USE OR INABILITY TO USE THE FONT SOFTWARE OR FROM OTHER DEALINGS IN THE FONT SOFTWARE.
 *
 * Except as contained in this notice, the names of Gnome, the Gnome Foundation, and Bitstream Inc., shall not be used in
 * advertising or otherwise to promote the sale, use or other dealings in this Font Software without prior written authorization
 * from the Gnome Foundation or Bitstream Inc., respectively."""


def find_ttf(name: str) -> str | None:
    for d in FONT_DIRS:
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    try:
        from PIL import ImageFont
        return ImageFont.truetype(name, 10).path          # PIL searches the platform's font directories for a bare name
    except (ImportError, OSError):
        pass
    try:
        import matplotlib
        p = os.path.join(os.path.dirname(matplotlib.__file__), "mpl-data", "fonts", "ttf", name)
        if os.path.exists(p):
            return p
    except ImportError:
        pass
    return None


def rasterise(path: str, size: int):
    """-> (advance, ascent, descent, rows[95 * (ascent + descent)])"""
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.truetype(path, size)
    asc0, desc0 = font.getmetrics()                     # PIL draws with the font's ascender at y = 0: baseline at y = asc0
    adv = int(round(font.getlength("M")))
    assert adv <= 32, adv
    H0 = asc0 + desc0 + 4
    cells = []
    for c in range(FIRST, LAST + 1):
        im = Image.new("L", (adv + 8, H0), 0)
        ImageDraw.Draw(im).text((0, 0), chr(c), font=font, fill=255)
        px = im.load()
        cells.append([[px[x, y] >= 128 for x in range(adv)] for y in range(H0)])
    ink = [y for cell in cells for y in range(H0) if any(cell[y])]
    top, bottom = min(ink), max(ink)
    ascent, descent = asc0 - top, bottom - asc0 + 1
    rows = []
    for cell in cells:
        for y in range(top, bottom + 1):
            rows.append(sum(1 << x for x in range(adv) if cell[y][x]))
    return adv, ascent, descent, rows


def render_header(fonts) -> str:
    out = ["/* font_atlas.h -- GENERATED by tools/gen_font_atlas.py; do not edit.",
           " *",
           " * 1-bit fonts of the frame renderer (csrc/render.hip), ASCII 32..126.  Glyph c occupies ATLAS_FONTn_ASCENT +",
           " * ATLAS_FONTn_DESCENT row words starting at (c - 32) * rows; row 0 lies ASCENT rows above the baseline; bit k of a",
           " * row word is column k of a cell ATLAS_FONTn_ADVANCE pixels wide.  Font 0: labels and zone names (cap height 10 px);",
           " * font 1: the HUD (bold, cap height 17 px).",
           " *",
           LICENCE,
           " */",
           "#ifndef ATLAS_FONT_ATLAS_H",
           "#define ATLAS_FONT_ATLAS_H",
           "",
           f"#define ATLAS_FONT_FIRST {FIRST}",
           f"#define ATLAS_FONT_COUNT {LAST - FIRST + 1}"]
    for i, (adv, asc, desc, rows) in enumerate(fonts):
        out += ["", f"#define ATLAS_FONT{i}_ADVANCE {adv}", f"#define ATLAS_FONT{i}_ASCENT {asc}", f"#define ATLAS_FONT{i}_DESCENT {desc}",
                f"#define ATLAS_FONT{i}_ROWS {{ \\"]
        H = asc + desc
        for g in range(LAST - FIRST + 1):
            words = ", ".join(f"0x{r:08x}u" for r in rows[g * H:(g + 1) * H])
            out.append(f"    {words}, /* {chr(FIRST + g)!r} */ \\".replace("/* '\\\\' */", "/* backslash */"))
        out.append("}")
    out += ["", "#endif /* ATLAS_FONT_ATLAS_H */", ""]
    return "\n".join(out)


def generate() -> str:
    fonts = []
    for name, size in FONTS:
        path = find_ttf(name)
        if path is None:
            raise FileNotFoundError(name)
        fonts.append(rasterise(path, size))
    return render_header(fonts)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with the committed header instead of writing it")
    ap.add_argument("--font-dir", action="append", default=[], help="directory holding the DejaVu Sans Mono TTF files (searched first)")
    args = ap.parse_args()
    FONT_DIRS[:0] = args.font_dir
    txt = generate()
    if args.check:
        same = open(OUT).read() == txt
        print("font_atlas.h is up to date" if same else "font_atlas.h differs from a fresh run")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(txt)
    print("wrote", OUT)
    return 0


if __name__ == "__main__":
    sys.exit(main())
