"""Writes df-vo_amd/csrc/vis_tables.h: the colour tables of the dense drawer panels, as data.

  * matplotlib's `magma` and `jet` as the drawer uses them: (cmap(arange(256))[:, :3] * 255).astype(uint8);
  * the Middlebury colour wheel (Baker et al., "A Database and Evaluation Methodology for Optical Flow"): 55 hues in the
    six segments RY 15, YG 6, GC 4, CB 11, BM 13, MR 6, each a ramp floor(255 * i / len) of one channel.

Run again only when the installed matplotlib changes its tables (tests/test_frame_drawer_cpu.py compares the header with it)."""
import os

import matplotlib
import numpy as np


def wheel():
    seg = [(15, 0, 1, +1), (6, 1, 0, -1), (4, 1, 2, +1), (11, 2, 1, -1), (13, 2, 0, +1), (6, 0, 2, -1)]  # len, full, ramp, sign
    rows = []
    for n, full, ramp, sign in seg:
        for i in range(n):
            c = [0, 0, 0]
            c[full] = 255
            r = (255 * i) // n
            c[ramp] = r if sign > 0 else 255 - r
            rows.append(c)
    return np.array(rows, np.uint8)


def table(name):
    cmap = matplotlib.colormaps[name]
    return (cmap(np.arange(256))[:, :3] * 255).astype(np.uint8)


def emit(f, name, a):
    f.write("static const unsigned char %s[%d][3] = {\n" % (name, len(a)))
    for i in range(0, len(a), 6):
        f.write("    " + " ".join("{%d, %d, %d}," % tuple(r) for r in a[i:i + 6]) + "\n")
    f.write("};\n")


def main():
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "df-vo_amd", "csrc", "vis_tables.h")
    with open(out, "w") as f:
        f.write("// Colour tables of the dense drawer panels (vis.hip) -- DATA, written by tools/gen_vis_tables.py.\n"
                "// VIS_TAB_MAGMA / VIS_TAB_JET: (cmap(arange(256))[:, :3] * 255).astype(uint8) of matplotlib %s;\n"
                "// VIS_TAB_WHEEL: the 55 Middlebury hues, RGB.\n#pragma once\n\n" % matplotlib.__version__)
        emit(f, "VIS_TAB_MAGMA", table("magma"))
        f.write("\n")
        emit(f, "VIS_TAB_JET", table("jet"))
        f.write("\n")
        emit(f, "VIS_TAB_WHEEL", wheel())


if __name__ == "__main__":
    main()
