#!/usr/bin/env python3
"""An equirectangular panorama of a named scene through trace_rays (needs an MI355X and Pillow): every pixel is the ray from one
point into the direction of its longitude and latitude - a picture the reference's pinhole camera (main.js:184-193) cannot make.

    python tools/panorama.py SCENE W H out.png [ox oy oz]

The eye defaults to the scene's camera origin.  Column x is the longitude 2 pi (x + 0.5) / W - pi measured from -z towards +x, row y
the latitude pi / 2 - pi (y + 0.5) / H: the centre of the picture looks along -z, as the reference's camera does.  Rays are listed
in row order, so neighbours in the list are neighbours in space, and a stars sky is the frame's (pix = y W + x).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "html5-canvas-raytracer_amd"))
import rt_host  # noqa: E402


def panorama_rays(w, h, eye):
    lon = 2.0 * np.pi * (np.arange(w) + 0.5) / w - np.pi
    lat = np.pi / 2.0 - np.pi * (np.arange(h) + 0.5) / h
    rays = np.empty((h, w, 6), np.float64)
    rays[..., 0:3] = np.asarray(eye, np.float64)
    rays[..., 3] = np.cos(lat)[:, None] * np.sin(lon)[None, :]
    rays[..., 4] = np.sin(lat)[:, None]
    rays[..., 5] = -np.cos(lat)[:, None] * np.cos(lon)[None, :]
    rays[..., 3:] = rt_host.normal3d(rays[..., 3:])
    return rays.reshape(h * w, 6)


def main(argv):
    from PIL import Image
    if len(argv) < 5:
        sys.exit(__doc__)
    name, w, h, out = argv[1], int(argv[2]), int(argv[3]), argv[4]
    scene = rt_host.load_scene(name)
    eye = [float(x) for x in argv[5:8]] if len(argv) >= 8 else scene["camera"]["origin"]
    rgba = rt_host.trace_rays(scene, panorama_rays(w, h, eye), want=("rgba",))["rgba"]
    Image.frombytes("RGBA", (w, h), rgba.tobytes()).convert("RGB").save(out)
    print("%s: %dx%d panorama from %s -> %s" % (name, w, h, eye, out))


if __name__ == "__main__":
    main(sys.argv)
