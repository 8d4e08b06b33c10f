#!/usr/bin/env python3
"""One light probe in a named scene: N rays leave the point (X, Y, Z) along the library's spiral over the whole sphere, each traced as the
reference traces any ray, and the probe's nine spherical-harmonics coefficients per channel are printed - rt_host.probes with
rt_host.sh9_weights, times 4 pi: the radiance coefficients a renderer lights a moving object with (needs an MI355X).

    python tools/probe.py SCENE X Y Z N [out.png]

N is the number of gathered rays (1..1024).  With out.png (needs Pillow) the N rays are also drawn as an equirectangular picture, 256 x
128, a 3 x 3 dot per ray at its longitude (atan2(y, x)) and latitude (asin(z)): the same N directions gathered one sample each - N
probes at the point, probe i taking table entry i (stride 1) - which gives every ray's own colour.
"""
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "html5-canvas-raytracer_amd"))
import rt_host  # noqa: E402

NAMES = ("1", "y", "z", "x", "xy", "yz", "xz", "3zz-1", "xx-yy")


def main(argv):
    if len(argv) not in (6, 7):
        sys.exit(__doc__)
    name, point, n = argv[1], [float(q) for q in argv[2:5]], int(argv[5])
    scene = rt_host.load_scene(name)
    dirs = rt_host.lighting_offsets(n)
    got = rt_host.probes(scene, [point], n, dirs=dirs, weights=rt_host.sh9_weights(dirs), want=("rgb", "coef"))
    print("%s: probe at %s, %d rays; mean colour %s" % (name, point, n, " ".join("%.4f" % c for c in got["rgb"][0])))
    for k, label in enumerate(NAMES):
        print("  L[%d] %-6s %s" % (k, label, " ".join("% .5f" % (4.0 * math.pi * c) for c in got["coef"][0, k])))
    if len(argv) == 7:
        from PIL import Image
        w, h = 256, 128
        rays = rt_host.gather(scene, rt_host.probe_records([point] * n), 1, dirs=dirs, stride=1, want=("rgba",), mapping="samples")["rgba"]
        img = Image.new("RGB", (w, h))
        for d, c in zip(dirs, rays):
            x = int((math.atan2(d[1], d[0]) / (2.0 * math.pi) + 0.5) * (w - 1))
            y = int((0.5 - math.asin(max(-1.0, min(1.0, d[2]))) / math.pi) * (h - 1))
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    img.putpixel(((x + dx) % w, min(max(y + dy, 0), h - 1)), (int(c[0]), int(c[1]), int(c[2])))
        img.save(argv[6])
        print("  the %d rays -> %s" % (n, argv[6]))


if __name__ == "__main__":
    main(sys.argv)
