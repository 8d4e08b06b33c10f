#!/usr/bin/env python3
"""A named scene lit by itself alone: per pixel of a pinhole view with the scene's camera, SAMPLES rays leave what the pixel sees over
the hemisphere of its facing normal, each is traced as the reference traces any ray (SEGS levels deep; default: the scene's depth), and
their mean colour is the pixel (rt_host.gather_view; needs an MI355X and Pillow) - the colour that bleeds onto a surface from its
surroundings, the sky light of a textured skybox, irradiance / pi.  Rays, hit records and gathered rays stay on the GPU: one launch per
band, 4 bytes per pixel come back.

    python tools/bleed.py SCENE W H out.png SAMPLES [SEGS]

SAMPLES is the number of gathered rays per pixel (1..1024).  The table is tools/ambient.py's: 61 copies of the library's cosine-weighted
SAMPLES-point spiral, copy j turned about the normal by j golden angles, and stride SAMPLES gives pixel i copy i % 61: every pixel
gathers over a whole well-spread set, and neighbours over different ones, which turns banding into noise.  The scene's lookAt basis is
used as it is, so the picture has the reference's handedness.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "html5-canvas-raytracer_amd"))
import rt_host  # noqa: E402
from ambient import COPIES, turned_copies  # noqa: E402


def main(argv):
    from PIL import Image
    if len(argv) not in (6, 7):
        sys.exit(__doc__)
    name, w, h, out, n = argv[1], int(argv[2]), int(argv[3]), argv[4], int(argv[5])
    segs = int(argv[6]) if len(argv) == 7 else 0
    scene = rt_host.load_scene(name)
    cam = scene["camera"]
    view = rt_host.view(rt_host.RT_VIEW_PINHOLE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], scene["fovDeg"])
    rgba = rt_host.gather_view(scene, view, w, h, n, dirs=turned_copies(rt_host.ambient_dirs(n), COPIES), stride=n, segs=segs)["rgba"]
    Image.frombytes("RGBA", (w, h), rgba.tobytes()).convert("RGB").save(out)
    print("%s: %dx%d, %d gathered rays per pixel, %s -> %s" % (name, w, h, n, "depth %d" % segs if segs else "the scene's depth", out))


if __name__ == "__main__":
    main(sys.argv)
