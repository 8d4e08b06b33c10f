"""TEST INFRASTRUCTURE for the tests of light moves on a resident scene (tests/test_lights_host.py, tests/test_gpu_lights.py): the
seeded light edits, and where a blob keeps its lights and their intensity.  The yardsticks are objects_util's: a fresh upload of the
edited blob, and the C restatement."""
import copy
import random
import struct

INTENSITY_OFFSET = 120          # rt_scene_header.light_intensity (include/rt_hip.h)
N_LIGHTS_OFFSET = 172           # rt_scene_header.n_lights
LIGHTS_OFFSET_OFFSET = 192      # rt_scene_header.lights_offset


def lights_offset(blob):
    return struct.unpack_from("<Q", blob, LIGHTS_OFFSET_OFFSET)[0]


def blob_lights(blob):
    n, off = struct.unpack_from("<I", blob, N_LIGHTS_OFFSET)[0], lights_offset(blob)
    return [list(struct.unpack_from("<3d", blob, off + 24 * k)) for k in range(n)]


def blob_intensity(blob):
    return struct.unpack_from("<d", blob, INTENSITY_OFFSET)[0]


def move_lights(scene, seed, swap=False):
    """A copy of `scene` with every light moved by a seeded uniform offset in +-2 per axis; `swap`: the first light then changes
    places with the last one."""
    s = copy.deepcopy(scene)
    rng = random.Random(seed)
    s["lights"] = [[c + rng.uniform(-2.0, 2.0) for c in l] for l in s["lights"]]
    if swap and len(s["lights"]) > 1:
        s["lights"][0], s["lights"][-1] = s["lights"][-1], s["lights"][0]
    return s


def set_lights(r, scene):
    r.set_lights(scene["lights"])
