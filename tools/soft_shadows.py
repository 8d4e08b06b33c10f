#!/usr/bin/env python3
"""A named scene as a picture of the light that arrives: per pixel of a pinhole view with the scene's camera, the reference's light loop
(main.js:283-306) N times with every light moved to a point of the sphere of radius RADIUS around it, min(1, mean diffuse sum) as a grey value
(rt_host.lighting_view; needs an MI355X and Pillow).  Rays, hit records and scans stay on the GPU: 4 bytes per pixel come back.

    python tools/soft_shadows.py SCENE W H out.png N RADIUS

N is the number of runs of the light loop per pixel (1..1024) and RADIUS the lights' radius in world units (0: point lights, hard
shadows - the reference's own loop).  The table holds 61 copies of the library's N-point spiral over the unit sphere, copy j turned about
z by j golden angles, and stride N gives pixel i copy i % 61: every pixel samples a whole well-spread set, and neighbours sample
different ones, which turns banding into noise.  (N consecutive entries of ONE long spiral would all lie on a ring.)  The scene's lookAt
basis is used as it is, so the picture has the reference's handedness.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "html5-canvas-raytracer_amd"))
import rt_host  # noqa: E402


COPIES = 61       # (a prime: the copies do not line up with the columns of a frame; 61 * 1024 entries fit the table's 65536)


def turned_copies(spiral, copies):
    """-> (copies * n, 3): the n offsets turned about z by j * pi * (3 - sqrt(5)), j = 0 .. copies - 1, back to back."""
    import numpy as np
    ang = np.arange(copies) * (np.pi * (3.0 - np.sqrt(5.0)))
    c, s = np.cos(ang)[:, None], np.sin(ang)[:, None]
    x, y, z = spiral[None, :, 0], spiral[None, :, 1], spiral[None, :, 2]
    return np.stack([c * x - s * y, s * x + c * y, np.broadcast_to(z, (copies, spiral.shape[0]))], axis=2).reshape(-1, 3)


def main(argv):
    from PIL import Image
    if len(argv) != 7:
        sys.exit(__doc__)
    name, w, h, out, n, radius = argv[1], int(argv[2]), int(argv[3]), argv[4], int(argv[5]), float(argv[6])
    scene = rt_host.load_scene(name)
    cam = scene["camera"]
    view = rt_host.view(rt_host.RT_VIEW_PINHOLE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], scene["fovDeg"])
    got = rt_host.lighting_view(scene, view, w, h, n, radius, offs=turned_copies(rt_host.lighting_offsets(n), COPIES), stride=n, want=("rgba", "lit"))
    Image.frombytes("RGBA", (w, h), got["rgba"].tobytes()).convert("RGB").save(out)
    lit = got["lit"]
    print("%s: %dx%d, %d samples per pixel of lights of radius %g -> %s (%d pixels lit by some but not all of their samples)"
          % (name, w, h, n, radius, out, int(((lit > 0) & (lit < 1)).sum())))


if __name__ == "__main__":
    main(sys.argv)
