#!/usr/bin/env python3
"""A named scene as the reference's own picture - colours, highlights, reflections, glass - with lights that have a size: the wavefront
trace of a pinhole view with the scene's camera, the diffuse and specular terms of its nodes averaged over N copies of the lights, each
moved to a point of the sphere of radius RADIUS around it (rt_host.trace_view_soft; needs an MI355X and Pillow).

    python tools/soft_picture.py SCENE W H out.png N RADIUS [LEVELS] [recursive]

N is the number of runs of the light loop per node (1..1024), RADIUS the lights' radius in world units (0: point lights, the hard
shadows of the reference) and LEVELS how many levels of the ray trees are relit: 1 (the default) softens what the camera sees directly,
the scene's depth every reflection and refraction as well.  The table is tools/soft_shadows.py's: 61 copies of the library's N-point
spiral over the unit sphere, copy j turned about z by j golden angles, and stride N gives pixel i copy i % 61 - every pixel samples a
whole well-spread set, neighbours sample different ones, and a pixel's bounces share its set.  The view's rays are made on the host and
cross the link (48 bytes each) - unless the last argument is `recursive`: then the rays are generated on the GPU and each chunk of rows
is one launch of the recursive soft kernel (rt_trace_view_soft), which draws the same bytes.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "html5-canvas-raytracer_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rt_host  # noqa: E402
from soft_shadows import COPIES, turned_copies  # noqa: E402


def main(argv):
    from PIL import Image
    recursive = argv[-1] == "recursive"
    if recursive:
        argv = argv[:-1]
    if len(argv) not in (7, 8):
        sys.exit(__doc__)
    name, w, h, out, n, radius = argv[1], int(argv[2]), int(argv[3]), argv[4], int(argv[5]), float(argv[6])
    levels = int(argv[7]) if len(argv) == 8 else 1
    scene = rt_host.load_scene(name)
    cam = scene["camera"]
    view = rt_host.view(rt_host.RT_VIEW_PINHOLE, cam["origin"], cam["axisX"], cam["axisY"], cam["axisZ"], scene["fovDeg"])
    got = rt_host.trace_view_soft(scene, view, w, h, n, radius, offs=turned_copies(rt_host.lighting_offsets(n), COPIES), stride=n, levels=levels,
                                  want=("rgba",) if recursive else ("rgba", "level_counts"), method="recursive" if recursive else "wavefront")
    hard = rt_host.trace_view_soft(scene, view, w, h, 1, 0.0, levels=0)
    Image.frombytes("RGBA", (w, h), got["rgba"].tobytes()).convert("RGB").save(out)
    changed = int((got["rgba"] != hard["rgba"]).any(axis=1).sum())
    traced = "one launch per chunk" if recursive else "%d nodes traced" % int(got["level_counts"].sum())
    print("%s: %dx%d, %d samples per node of lights of radius %g on %d level(s) -> %s (%s; %d pixels differ from the point-light picture)"
          % (name, w, h, n, radius, levels, out, traced, changed))


if __name__ == "__main__":
    main(sys.argv)
