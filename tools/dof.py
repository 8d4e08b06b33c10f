#!/usr/bin/env python3
"""A named scene through a thin lens, antialiased: k x k samples per pixel of a pinhole view with the scene's camera, averaged on the
GPU (rt_host.trace_view_samples; needs an MI355X and Pillow).  The reference's camera (main.js:184-193) has neither.

    python tools/dof.py SCENE W H out.png K RADIUS FOCUS

K is the grid (1..32: K K samples per pixel, sub-pixel offsets and lens points from one pattern, rt_host.view_samples_grid), RADIUS the
lens' radius in world units (0: antialiasing only), FOCUS the distance of the plane that stays sharp, along the camera's axis_z.  The
scene's lookAt basis is used as it is, so the picture has the reference's handedness.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "html5-canvas-raytracer_amd"))
import rt_host  # noqa: E402


def main(argv):
    from PIL import Image
    if len(argv) != 8:
        sys.exit(__doc__)
    name, w, h, out, k, radius, focus = argv[1], int(argv[2]), int(argv[3]), argv[4], int(argv[5]), float(argv[6]), float(argv[7])
    scene = rt_host.load_scene(name)
    cam = scene["camera"]
    view = rt_host.view(rt_host.RT_VIEW_PINHOLE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], scene["fovDeg"])
    lens = rt_host.lens(radius, focus) if radius > 0 else None
    rgba = rt_host.trace_view_samples(scene, view, w, h, rt_host.view_samples_grid(k), lens=lens)["rgba"]
    Image.frombytes("RGBA", (w, h), rgba.tobytes()).convert("RGB").save(out)
    print("%s: %dx%d, %d samples per pixel, lens radius %g focused at %g -> %s" % (name, w, h, k * k, radius, focus, out))


if __name__ == "__main__":
    main(sys.argv)
