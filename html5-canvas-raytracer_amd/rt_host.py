"""Python host side of the MI355X ray-sphere path: scene loading/flattening and the ctypes
binding of the C ABI in include/rt_hip.h.

This mirrors what the Node host (js/index.js + napi/rt_napi.cc) does, for the Python callers
the build contract requires (pytest, bench.py, __graft_entry__).  It contains NO rendering
code and no CPU fallback: every render goes through librt_hip.so -> the HIP kernel, and
`load_library()` raises if that library is missing.

Scene schema = the reference's locals/literals (main.js:85-163, :194, :283-284), see
js/scene.js; blob layout = include/rt_hip.h (rt_scene_header + tables).
"""
import base64
import ctypes as C
import json
import numbers
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCENES_DIR = os.path.join(HERE, "scenes")
LIB_PATH = os.environ.get("RT_HIP_LIB") or os.path.join(HERE, "csrc", "librt_hip.so")   # RT_HIP_LIB: A/B builds
# The TEST build of the same sources (-DRT_TESTING): the only library that reads the A/B and test environment switches
# (RT_EMULATE_DEVICES, RT_NO_BOUNCE_TABLE, RT_NO_FIXUP, ...) and exports rt_test_probe.  Tests select it with RT_HIP_LIB.
TEST_LIB_PATH = os.path.join(HERE, "csrc", "librt_hip_test.so")

RT_SCENE_MAGIC = 0x31535452
RT_ABI_VERSION = 2
HEADER_BYTES, SPHERE_BYTES, TEXDESC_BYTES = 208, 192, 16
SAMPLER_COLOR, SAMPLER_TEXTURE, SAMPLER_CHECKER, SAMPLER_STARS = 0, 1, 2, 3

RT_FLAG_COUNT = 1
RT_FLAG_STRICT_FP = 2
RT_FLAG_RGB24 = 4        # device entry points: 3 bytes per pixel, the constant alpha stays home (include/rt_hip.h)
RT_FLAG_NO_SKY = 8       # blocks that can only show the constant background are not stored (the frame's owner stores them: RT_FLAG_SKY_ONLY)
RT_FLAG_SKY_ONLY = 16
RT_FLAG_COMPACT = 32     # with RT_FLAG_RGB24 | RT_FLAG_NO_SKY: a compact band (the stored blocks back to back, for a collective)
RT_FLAG_STARS_PER_FRAME = 64   # batches: frame f draws its stars with seed starsSeed + f (mod 2^32); without it every frame is the same


# --------------------------------------------------------------------------- scenes
def load_scene(name_or_path):
    """Load a scene JSON written by js/flatten.js sceneToJSON (textures resolved to bytes)."""
    path = name_or_path
    if not os.path.isabs(path) and not os.path.exists(path):
        path = os.path.join(SCENES_DIR, name_or_path + ".json")
    with open(path) as f:
        scene = json.load(f)
    d = os.path.dirname(os.path.abspath(path))
    for t in scene["textures"]:
        if "base64" in t:
            t["texels"] = base64.b64decode(t.pop("base64"))
        else:
            with open(os.path.join(d, t["file"]), "rb") as f:
                t["texels"] = f.read()
        if len(t["texels"]) != t["width"] * t["height"] * 4:
            raise ValueError("texture is not width*height*4 bytes of RGBA8")
    return scene


def validate_scene(scene):
    """Host-side checks, same rules as js/scene.js validateScene."""
    cam = scene["camera"]
    for k in ("origin", "axisX", "axisY", "axisZ"):
        if len(cam[k]) != 3:
            raise ValueError("scene.camera.%s must be a 3-vector" % k)
    if not (isinstance(scene["segs"], int) and 0 <= scene["segs"] <= 16):
        raise ValueError("scene.segs must be an integer in [0,16]")
    if scene.get("supersample", 1) not in (1, 2, 3, 4):
        raise ValueError("scene.supersample must be 1, 2, 3 or 4")
    if not (1 <= len(scene["objects"]) <= 256):
        raise ValueError("scene.objects must hold 1..256 spheres")
    if len(scene["lights"]) > 16:
        raise ValueError("scene.lights must hold 0..16 lights")
    if len(scene["textures"]) > 16:
        raise ValueError("scene.textures must hold 0..16 textures")
    for i, t in enumerate(scene["textures"]):
        if not (1 <= t["width"] <= 16384 and 1 <= t["height"] <= 16384):
            raise ValueError("texture %d: width and height must be in 1..16384" % i)
    seed = scene.get("starsSeed", 0)
    if not (isinstance(seed, int) and not isinstance(seed, bool) and 0 <= seed < 2 ** 32):
        raise ValueError("scene.starsSeed must be an integer in [0, 2^32)")
    for i, o in enumerate(scene["objects"]):
        s = o["mtl"]["sampler"]
        if s["kind"] not in (SAMPLER_COLOR, SAMPLER_TEXTURE, SAMPLER_CHECKER, SAMPLER_STARS):
            raise ValueError("object %d: unsupported sampler kind %r (0 colour, 1 texture, 2 checker, 3 hashed stars)" % (i, s["kind"]))
        if s["kind"] == SAMPLER_TEXTURE and not (0 <= s["texture"] < len(scene["textures"])):
            raise ValueError("object %d: texture index out of range" % i)


def _sphere_record(ob):
    m = ob["mtl"]
    s = m["sampler"]
    if s["kind"] == SAMPLER_CHECKER:
        ck = [s["freqU"], s["freqV"], *s["colors"][0], *s["colors"][1]]
    elif s["kind"] == SAMPLER_STARS:
        ck = [s["threshold"], s["scale"], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    else:
        ck = [0.0] * 8
    rec = struct.pack("<22d2id", *ob["origin"], ob["r2"], *m["color"], m["specular_exponent"],
                      *m["albedo"], m["refract_index"], *[float(x) for x in ck],
                      s["kind"], s["texture"] if s["kind"] == SAMPLER_TEXTURE else -1, 0.0)
    assert len(rec) == SPHERE_BYTES
    return rec


def sphere_records(objects):
    """scene-dict objects -> their rt_sphere records (bytes, SPHERE_BYTES each), packed exactly as flatten_scene packs them: what
    rt_scene_set_objects / Renderer.set_objects take."""
    return b"".join(_sphere_record(ob) for ob in objects)


def light_positions(lights):
    """A list of 3-vectors -> its numbers in order (3 floats per light), as flatten_scene packs a scene's lights: what
    rt_scene_set_lights / Renderer.set_lights take.  ValueError for anything else."""
    if isinstance(lights, (str, bytes, bytearray)) or not hasattr(lights, "__len__") or not hasattr(lights, "__getitem__"):
        raise ValueError("lights must be a list of 3-vectors")
    flat = []
    for l in lights:
        if isinstance(l, (str, bytes, bytearray)) or not hasattr(l, "__len__") or len(l) != 3:
            raise ValueError("a light is a 3-vector [x, y, z]")
        for c in l:
            if isinstance(c, bool) or not isinstance(c, numbers.Real):
                raise ValueError("a light's coordinates are numbers")
            flat.append(float(c))
    return flat


def flatten_scene(scene):
    """scene dict -> pointer-free blob (bytes), byte-identical to js/flatten.js flattenScene."""
    validate_scene(scene)
    objs, lights, texs = scene["objects"], scene["lights"], scene["textures"]
    objects_off = HEADER_BYTES
    lights_off = objects_off + len(objs) * SPHERE_BYTES
    tex_off = lights_off + len(lights) * 24
    cursor = tex_off + len(texs) * TEXDESC_BYTES
    texel_off = []
    for t in texs:
        texel_off.append(cursor)
        cursor += (len(t["texels"]) + 7) & ~7
    total = cursor
    cam = scene["camera"]
    out = bytearray(total)
    hdr = struct.pack(
        "<IIQ12d3d3dIIIIIIQQQ", RT_SCENE_MAGIC, RT_ABI_VERSION, total,
        *cam["origin"], *cam["axisX"], *cam["axisY"], *cam["axisZ"],
        float(scene.get("fovDeg", 60)), float(scene.get("light_intensity", 50)), float(scene.get("epsilon", 0.001)),
        *[float(x) for x in scene.get("miss_color", [1, 0, 0])],
        scene["segs"], scene.get("supersample", 1), len(objs), len(lights), len(texs), scene.get("starsSeed", 0),
        objects_off, lights_off, tex_off)
    assert len(hdr) == HEADER_BYTES
    out[0:HEADER_BYTES] = hdr
    o = objects_off
    out[o:o + len(objs) * SPHERE_BYTES] = sphere_records(objs)
    o += len(objs) * SPHERE_BYTES
    for l in lights:
        out[o:o + 24] = struct.pack("<3d", *l)
        o += 24
    for t, off in zip(texs, texel_off):
        out[o:o + TEXDESC_BYTES] = struct.pack("<IIQ", t["width"], t["height"], off)
        o += TEXDESC_BYTES
    for t, off in zip(texs, texel_off):
        out[off:off + len(t["texels"])] = t["texels"]
    return bytes(out)


# --------------------------------------------------------------------------- C ABI binding
class RtTiles(C.Structure):
    _fields_ = [("tile_rows", C.c_uint32), ("tile_first", C.c_uint32), ("tile_stride", C.c_uint32), ("n_tiles", C.c_uint32)]


class RtStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("pixels", C.c_uint64), ("rays", C.c_uint64),
                ("shadow_rays", C.c_uint64), ("sphere_tests", C.c_uint64), ("exact_samples", C.c_uint64)]


class RtHit(C.Structure):
    """A primary hit (include/rt_hip.h rt_hit, 80 bytes): main.js:440-449's hit_i, inside flag, t, p, n, u, v."""
    _fields_ = [("object", C.c_int32), ("inside", C.c_int32), ("t", C.c_double), ("point", C.c_double * 3), ("normal", C.c_double * 3),
                ("u", C.c_double), ("v", C.c_double)]


class RtHitBuffers(C.Structure):
    _fields_ = [("id", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p)]


class RtRayOutputs(C.Structure):
    """Outputs of a ray list (include/rt_hip.h rt_ray_outputs): 3 float64, 4 uint8, one RtHit per ray; NULL = not wanted."""
    _fields_ = [("rgb", C.c_void_p), ("rgba", C.c_void_p), ("hits", C.c_void_p)]


class RtOcclusionInputs(C.Structure):
    """Per-ray inputs of an occlusion query (include/rt_hip.h rt_occlusion_inputs): float64 length, float64 intensity, int32 skip; NULL =
    +Infinity / the scene's light intensity / no sphere left out."""
    _fields_ = [("length", C.c_void_p), ("intensity", C.c_void_p), ("skip", C.c_void_p)]


class RtOcclusionOutputs(C.Structure):
    """Outputs of an occlusion query (include/rt_hip.h rt_occlusion_outputs): float64 intensity, int32 blocker per ray; NULL = not wanted."""
    _fields_ = [("intensity", C.c_void_p), ("blocker", C.c_void_p)]


RT_VIEW_REFERENCE, RT_VIEW_PINHOLE, RT_VIEW_ORTHO, RT_VIEW_EQUIRECT = 0, 1, 2, 3


class RtView(C.Structure):
    """A camera model (include/rt_hip.h rt_view, 136 bytes): model, origin, three axes, fov_deg (the perspective models), scale (ORTHO),
    and the panorama's two tables (EQUIRECT: host memory for the host forms, device memory for the Renderer's)."""
    _fields_ = [("model", C.c_uint32), ("reserved", C.c_uint32), ("origin", C.c_double * 3), ("axis_x", C.c_double * 3), ("axis_y", C.c_double * 3),
                ("axis_z", C.c_double * 3), ("fov_deg", C.c_double), ("scale", C.c_double), ("lon", C.c_void_p), ("lat", C.c_void_p)]


class RtViewSample(C.Structure):
    """One sample of a sampled view (include/rt_hip.h rt_view_sample, 32 bytes): the sub-pixel offset (dx, dy) in pixels, dy downwards,
    and the lens point (lu, lv) on the unit disk."""
    _fields_ = [("dx", C.c_double), ("dy", C.c_double), ("lu", C.c_double), ("lv", C.c_double)]


class RtViewLens(C.Structure):
    """A thin lens for RT_VIEW_PINHOLE (include/rt_hip.h rt_view_lens): its radius and the distance of the plane of focus along axis_z."""
    _fields_ = [("radius", C.c_double), ("focus", C.c_double)]


class RtAmbient(C.Structure):
    """Ambient occlusion (include/rt_hip.h struct rt_ambient, 32 bytes): n_samples scans per receiver, the direction table's n_dirs
    entries, the stride and base of the entry index e = ((base + i) * stride + s) % n_dirs, and the scans' length `radius`."""
    _fields_ = [("n_samples", C.c_uint32), ("n_dirs", C.c_uint32), ("stride", C.c_uint32), ("reserved", C.c_uint32), ("base", C.c_uint64),
                ("radius", C.c_double)]


class RtAmbientOutputs(C.Structure):
    """Outputs of ambient occlusion (include/rt_hip.h rt_ambient_outputs): float64 open, float64 intensity, uint32 rgba per receiver;
    NULL = not wanted."""
    _fields_ = [("open", C.c_void_p), ("intensity", C.c_void_p), ("rgba", C.c_void_p)]


class RtLighting(C.Structure):
    """Sampled lights (include/rt_hip.h struct rt_lighting, 32 bytes): n_samples runs of the light loop per receiver, the offset table's
    n_offs entries, the stride and base of the entry index e = ((base + i) * stride + s) % n_offs, and the lights' radius."""
    _fields_ = [("n_samples", C.c_uint32), ("n_offs", C.c_uint32), ("stride", C.c_uint32), ("reserved", C.c_uint32), ("base", C.c_uint64),
                ("light_radius", C.c_double)]


class RtLightingOutputs(C.Structure):
    """Outputs of sampled lights (include/rt_hip.h rt_lighting_outputs): float64 diffuse, float64 intensity, float64 lit, uint32 rgba per
    receiver; NULL = not wanted."""
    _fields_ = [("diffuse", C.c_void_p), ("intensity", C.c_void_p), ("lit", C.c_void_p), ("rgba", C.c_void_p)]


class RtGather(C.Structure):
    """Gathered light (include/rt_hip.h struct rt_gather, 32 bytes): n_samples rays per receiver, the direction table's n_dirs entries,
    the stride and base of the entry index e = ((base + i) * stride + s) % n_dirs, the depth `segs` of every gathered ray (0: the scene's)
    and the stars sampler's pix = pix_base + s * pix_stride + i."""
    _fields_ = [("n_samples", C.c_uint32), ("n_dirs", C.c_uint32), ("stride", C.c_uint32), ("segs", C.c_uint32), ("base", C.c_uint64),
                ("pix_base", C.c_uint32), ("pix_stride", C.c_uint32)]


class RtGatherOutputs(C.Structure):
    """Outputs of gathered light (include/rt_hip.h rt_gather_outputs): 3 float64 rgb, uint32 rgba per receiver; NULL = not wanted."""
    _fields_ = [("rgb", C.c_void_p), ("rgba", C.c_void_p)]


class RtProbeOutputs(C.Structure):
    """Outputs of the probe call (include/rt_hip.h rt_probe_outputs): rgb and rgba as RtGatherOutputs, coef n x n_weights x 3 float64;
    NULL = not wanted."""
    _fields_ = [("rgb", C.c_void_p), ("rgba", C.c_void_p), ("coef", C.c_void_p)]


# every symbol include/rt_hip.h declares: (restype, argtypes)
ABI = {
    "rt_init": (C.c_int, [C.c_int]),
    "rt_shutdown": (None, []),
    "rt_device_count": (C.c_int, []),
    "rt_last_error": (C.c_char_p, []),
    "rt_abi_version": (C.c_uint32, []),
    "rt_build_id": (C.c_char_p, []),
    "rt_elapsed_report": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "rt_scene_validate": (C.c_int, [C.c_void_p, C.c_size_t]),
    "rt_scene_cull_rects": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_double)]),
    "rt_scene_bounce_candidates": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "rt_scene_launch_table": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(RtTiles), C.c_int, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rt_scene_upload": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "rt_scene_free": (None, [C.c_void_p]),
    "rt_scene_set_camera": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p]),
    "rt_scene_set_stars_seed": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rt_scene_trace_occupancy": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "rt_scene_set_objects": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_scene_set_lights": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.c_void_p]),
    "rt_scene_set_light_intensity": (C.c_int, [C.c_void_p, C.c_double]),
    "rt_scene_set_texels": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rt_scene_set_texels_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rt_render_tiles_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(RtTiles), C.c_void_p, C.c_void_p,
                                         C.c_uint32, C.POINTER(RtStats)]),
    "rt_render_batch_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(RtTiles), C.c_uint32, C.c_void_p, C.c_uint64,
                                         C.c_void_p, C.c_uint32, C.POINTER(RtStats)]),
    "rt_render": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(RtStats)]),
    "rt_render_progressive": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                        C.POINTER(RtStats)]),
    "rt_render_options": (C.c_int, [C.c_int, C.c_uint32]),
    "rt_alloc_pinned": (C.c_void_p, [C.c_size_t]),
    "rt_free_pinned": (None, [C.c_void_p]),
    "rt_alloc_device": (C.c_void_p, [C.c_int, C.c_size_t]),
    "rt_free_device": (None, [C.c_int, C.c_void_p]),
    "rt_copy_to_host": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rt_deinterleave_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_uint64, C.c_void_p]),
    "rt_memset_device": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_size_t]),
    "rt_render_scatter_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(RtTiles), C.c_uint32, C.POINTER(C.c_void_p), C.c_void_p,
                                           C.c_uint32, C.POINTER(RtStats)]),
    "rt_ipc_export": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p]),
    "rt_ipc_open": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    "rt_ipc_close": (C.c_int, [C.c_int, C.c_void_p]),
    "rt_compact_count": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rt_compact_expand_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_deinterleave_rgb24_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.c_uint64, C.c_void_p]),
    "rt_render_hits_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(RtTiles), C.POINTER(RtHitBuffers), C.c_void_p,
                                        C.POINTER(RtStats)]),
    "rt_adaptive_work_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rt_render_adaptive_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.c_uint32, C.POINTER(RtStats)]),
    "rt_render_adaptive": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.POINTER(RtStats), C.POINTER(C.c_uint64)]),
    "rt_scene_pick": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(RtHit)]),
    "rt_render_hits": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(RtHitBuffers), C.POINTER(RtStats)]),
    "rt_pick": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(RtHit)]),
    "rt_scene_trace_rays_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(RtRayOutputs), C.c_void_p, C.POINTER(RtStats)]),
    "rt_trace_rays": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(RtRayOutputs), C.POINTER(RtStats)]),
    "rt_rays_order_work_bytes": (C.c_size_t, [C.c_uint64]),
    "rt_scene_order_rays_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rt_scene_trace_rays_ordered_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(RtRayOutputs), C.c_void_p,
                                                     C.POINTER(RtStats)]),
    "rt_trace_rays_binned": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(RtRayOutputs), C.POINTER(RtStats)]),
    "rt_scene_occlusion_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(RtOcclusionInputs), C.POINTER(RtOcclusionOutputs),
                                            C.c_void_p, C.POINTER(RtStats)]),
    "rt_occlusion": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.POINTER(RtOcclusionInputs), C.POINTER(RtOcclusionOutputs), C.POINTER(RtStats)]),
    "rt_occlusion_binned": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.POINTER(RtOcclusionInputs), C.POINTER(RtOcclusionOutputs),
                                      C.POINTER(RtStats)]),
    "rt_scene_shade_rays_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(RtStats)]),
    "rt_shade_rays": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(RtStats)]),
    "rt_nodes_spawn_work_bytes": (C.c_size_t, [C.c_uint64]),
    "rt_scene_spawn_rays_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rt_scene_fold_nodes_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_trace_rays_wavefront": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(RtRayOutputs), C.POINTER(RtStats),
                                          C.POINTER(C.c_uint64)]),
    "rt_view_validate": (C.c_int, [C.POINTER(RtView), C.c_uint32, C.c_uint32]),
    "rt_view_equirect_tables": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_view_rays": (C.c_int, [C.POINTER(RtView), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "rt_view_rays_device": (C.c_int, [C.c_int, C.POINTER(RtView), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_view_work_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rt_scene_trace_view_device": (C.c_int, [C.c_void_p, C.POINTER(RtView), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RtRayOutputs), C.c_void_p,
                                             C.c_size_t, C.c_void_p, C.POINTER(RtStats)]),
    "rt_trace_view": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(RtView), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RtRayOutputs), C.POINTER(RtStats)]),
    "rt_view_samples_validate": (C.c_int, [C.POINTER(RtView), C.c_uint32, C.c_uint32, C.POINTER(RtViewLens), C.c_uint32, C.c_void_p]),
    "rt_view_samples_grid": (C.c_int, [C.c_uint32, C.c_void_p]),
    "rt_view_equirect_sample_tables": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_view_sample_rays": (C.c_int, [C.POINTER(RtView), C.c_uint32, C.c_uint32, C.POINTER(RtViewLens), C.POINTER(RtViewSample), C.c_uint32, C.c_uint32,
                                      C.c_uint32, C.c_void_p]),
    "rt_view_sample_rays_device": (C.c_int, [C.c_int, C.POINTER(RtView), C.c_uint32, C.c_uint32, C.POINTER(RtViewLens), C.POINTER(RtViewSample), C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_view_samples_work_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rt_scene_trace_view_samples_device": (C.c_int, [C.c_void_p, C.POINTER(RtView), C.c_uint32, C.c_uint32, C.POINTER(RtViewLens), C.c_uint32, C.c_void_p,
                                                     C.c_uint32, C.POINTER(RtRayOutputs), C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(RtStats)]),
    "rt_trace_view_samples": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(RtView), C.c_uint32, C.c_uint32, C.POINTER(RtViewLens), C.c_uint32, C.c_void_p,
                                        C.c_uint32, C.POINTER(RtRayOutputs), C.POINTER(RtStats)]),
    "rt_ambient_validate": (C.c_int, [C.POINTER(RtAmbient), C.c_void_p]),
    "rt_ambient_cosine_dirs": (C.c_int, [C.c_uint32, C.c_void_p]),
    "rt_ambient_segments": (C.c_int, [C.POINTER(RtAmbient), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_ambient_segments_device": (C.c_int, [C.c_int, C.POINTER(RtAmbient), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "rt_scene_ambient_device": (C.c_int, [C.c_void_p, C.POINTER(RtAmbient), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(RtAmbientOutputs),
                                          C.c_void_p, C.POINTER(RtStats)]),
    "rt_ambient": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(RtAmbient), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(RtAmbientOutputs),
                             C.POINTER(RtStats)]),
    "rt_ambient_view_work_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rt_scene_ambient_view_device": (C.c_int, [C.c_void_p, C.POINTER(RtView), C.c_uint32, C.c_uint32, C.POINTER(RtAmbient), C.c_void_p,
                                               C.POINTER(RtAmbientOutputs), C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(RtStats)]),
    "rt_ambient_view": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(RtView), C.c_uint32, C.c_uint32, C.POINTER(RtAmbient), C.c_void_p,
                                  C.POINTER(RtAmbientOutputs), C.POINTER(RtStats)]),
    "rt_lighting_validate": (C.c_int, [C.POINTER(RtLighting), C.c_void_p]),
    "rt_lighting_sphere_offsets": (C.c_int, [C.c_uint32, C.c_void_p]),
    "rt_lighting_segments": (C.c_int, [C.POINTER(RtLighting), C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_scene_lighting_device": (C.c_int, [C.c_void_p, C.POINTER(RtLighting), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(RtLightingOutputs),
                                           C.c_void_p, C.POINTER(RtStats)]),
    "rt_lighting": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(RtLighting), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(RtLightingOutputs),
                              C.POINTER(RtStats)]),
    "rt_lighting_view_work_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rt_scene_lighting_view_device": (C.c_int, [C.c_void_p, C.POINTER(RtView), C.c_uint32, C.c_uint32, C.POINTER(RtLighting), C.c_void_p,
                                                C.POINTER(RtLightingOutputs), C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(RtStats)]),
    "rt_lighting_view": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(RtView), C.c_uint32, C.c_uint32, C.POINTER(RtLighting), C.c_void_p,
                                   C.POINTER(RtLightingOutputs), C.POINTER(RtStats)]),
    "rt_scene_relight_nodes_device": (C.c_int, [C.c_void_p, C.POINTER(RtLighting), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.POINTER(RtStats)]),
    "rt_relight_rays": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(RtLighting), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_void_p, C.POINTER(RtStats)]),
    "rt_trace_rays_soft": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(RtLighting), C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int,
                                     C.POINTER(RtRayOutputs), C.POINTER(RtStats), C.POINTER(C.c_uint64)]),
    "rt_scene_trace_rays_soft_device": (C.c_int, [C.c_void_p, C.POINTER(RtLighting), C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                                  C.c_uint32, C.POINTER(RtRayOutputs), C.c_void_p, C.POINTER(RtStats)]),
    "rt_soft_view_work_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rt_scene_trace_view_soft_device": (C.c_int, [C.c_void_p, C.POINTER(RtView), C.c_uint32, C.c_uint32, C.POINTER(RtLighting), C.c_void_p, C.c_uint32,
                                                  C.c_uint32, C.POINTER(RtRayOutputs), C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(RtStats)]),
    "rt_trace_rays_soft_recursive": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(RtLighting), C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32,
                                               C.c_int, C.POINTER(RtRayOutputs), C.POINTER(RtStats)]),
    "rt_trace_view_soft": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(RtView), C.c_uint32, C.c_uint32, C.POINTER(RtLighting), C.c_void_p, C.c_uint32,
                                     C.c_uint32, C.POINTER(RtRayOutputs), C.POINTER(RtStats)]),
    "rt_gather_validate": (C.c_int, [C.POINTER(RtGather), C.c_void_p]),
    "rt_scene_gather_device": (C.c_int, [C.c_void_p, C.POINTER(RtGather), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(RtGatherOutputs),
                                         C.c_void_p, C.POINTER(RtStats)]),
    "rt_gather": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(RtGather), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(RtGatherOutputs),
                            C.POINTER(RtStats)]),
    "rt_gather_view_work_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rt_scene_gather_view_device": (C.c_int, [C.c_void_p, C.POINTER(RtView), C.c_uint32, C.c_uint32, C.POINTER(RtGather), C.c_void_p,
                                              C.POINTER(RtGatherOutputs), C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(RtStats)]),
    "rt_gather_view": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(RtView), C.c_uint32, C.c_uint32, C.POINTER(RtGather), C.c_void_p,
                                 C.POINTER(RtGatherOutputs), C.POINTER(RtStats)]),
    "rt_probes_validate": (C.c_int, [C.POINTER(RtGather), C.c_void_p, C.c_void_p, C.c_uint32]),
    "rt_probe_sh9_weights": (C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p]),
    "rt_scene_gather_probes_device": (C.c_int, [C.c_void_p, C.POINTER(RtGather), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p,
                                                C.POINTER(RtProbeOutputs), C.c_void_p, C.POINTER(RtStats)]),
    "rt_gather_probes": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(RtGather), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p,
                                   C.POINTER(RtProbeOutputs), C.POINTER(RtStats)]),
}

RT_PROBE_MAX_WEIGHTS = 16

RT_MAX_SEGS = 16

# include/rt_hip.h rt_hit (80 bytes) and rt_node (200 bytes) as numpy fields, in the header's order; NODE_DTYPE (below) is the structured dtype
HIT_FIELDS = [("object", "<i4"), ("inside", "<i4"), ("t", "<f8"), ("point", "<f8", (3,)), ("normal", "<f8", (3,)), ("u", "<f8"), ("v", "<f8")]
NODE_FIELDS = [("object", "<i4"), ("inside", "<i4"), ("t", "<f8"), ("point", "<f8", (3,)), ("normal", "<f8", (3,)), ("u", "<f8"), ("v", "<f8"),
               ("sample", "<f8", (3,)), ("diffuse", "<f8"), ("specular", "<f8"), ("ambient", "<f8"), ("reflect_weight", "<f8"),
               ("refract_weight", "<f8"), ("reflect_dir", "<f8", (3,)), ("refract_dir", "<f8", (3,)), ("children", "<u4"), ("reserved", "<u4")]


class RtError(RuntimeError):
    pass


_lib = None


def load_library(path=None):
    """dlopen librt_hip.so and type every entry point.  No fallback: a missing library is an error."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RtError("HIP library %s is missing - run `python -c 'import __graft_entry__ as g; g.build()'`; "
                      "there is no CPU fallback for the render path" % p)
    lib = C.CDLL(p)
    older = os.environ.get("RT_HIP_LIB_OLDER") == "1"    # A/B runs against a library built from an older revision (profiles/ab_run.sh)
    for name, (res, args) in ABI.items():
        if older and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)        # AttributeError if the library does not export it
        fn.restype, fn.argtypes = res, args
    if path is None:
        _lib = lib
    return lib


def _check(lib, rc, what):
    if rc != 0:
        msg = lib.rt_last_error()
        raise RtError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


class Renderer:
    """A scene resident on one GPU.  render_tiles() writes into caller-provided DEVICE memory
    (a torch uint8 CUDA tensor's data_ptr, or rt_alloc_device memory)."""

    def __init__(self, scene, device=0, lib=None):
        self.lib = lib or load_library()
        self.blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
        self.device = device
        if self.lib.rt_device_count() < 0:          # not initialised yet: use every visible GPU (an earlier rt_init's choice stands)
            _check(self.lib, self.lib.rt_init(0), "rt_init")
        h = C.c_void_p()
        buf = C.create_string_buffer(self.blob, len(self.blob))
        _check(self.lib, self.lib.rt_scene_upload(device, buf, len(self.blob), C.byref(h)), "rt_scene_upload")
        self.handle = h

    def set_camera(self, camera, stream=None):
        """Move the camera of the resident scene (lookAt, main.js:92-100): `camera` = {"origin", "axisX", "axisY", "axisZ"}.  One small
        asynchronous copy; the next render rebuilds what depends on it on the GPU."""
        v = [(C.c_double * 3)(*camera[k]) for k in ("origin", "axisX", "axisY", "axisZ")]
        _check(self.lib, self.lib.rt_scene_set_camera(self.handle, v[0], v[1], v[2], v[3], C.c_void_p(stream or 0)), "rt_scene_set_camera")

    def set_stars_seed(self, seed):
        """Seed of the stars sampler's hash for the scene's later renders (the reference's new Math.random() draws per redraw,
        main.js:135-139, 180).  Host state only: renders already enqueued keep the seed they were launched with."""
        if not (isinstance(seed, int) and not isinstance(seed, bool) and 0 <= seed < 2 ** 32):
            raise ValueError("stars seed must be an integer in [0, 2^32)")
        _check(self.lib, self.lib.rt_scene_set_stars_seed(self.handle, seed), "rt_scene_set_stars_seed")

    def trace_occupancy(self, four_waves=False):
        """(workgroups of the scene's trace kernel that one compute unit holds at once, dynamic LDS bytes per workgroup) for a colour launch
        of the resident scene, by the HIP runtime's occupancy count; `four_waves`: the first frame from a moved camera.  Launches nothing."""
        n, lds = C.c_int(), C.c_uint32()
        _check(self.lib, self.lib.rt_scene_trace_occupancy(self.handle, 1 if four_waves else 0, C.byref(n), C.byref(lds)), "rt_scene_trace_occupancy")
        return n.value, lds.value

    def set_objects(self, objects, first=0, stream=None):
        """Replace spheres [first, first + len(objects)) of the resident scene (scene-dict objects, or their packed records from
        sphere_records): asynchronous, like a camera move; the next render sees them.  RtError (RT_ERR_UNSUPPORTED) when the edit
        changes the sphere that encloses everything: upload the scene again."""
        recs = bytes(objects) if isinstance(objects, (bytes, bytearray)) else sphere_records(objects)
        if len(recs) % SPHERE_BYTES:
            raise ValueError("sphere records are %d bytes each" % SPHERE_BYTES)
        buf = C.create_string_buffer(recs, max(len(recs), 1))
        _check(self.lib, self.lib.rt_scene_set_objects(self.handle, first, len(recs) // SPHERE_BYTES, buf, C.c_void_p(stream or 0)),
               "rt_scene_set_objects")

    def set_lights(self, lights, first=0, stream=None):
        """Move lights [first, first + len(lights)) of the resident scene (a list of 3-vectors; the reference's literal array,
        main.js:283): asynchronous, like an object move and cheaper; the next render sees them.  RtError (RT_ERR_UNSUPPORTED) when the
        move changes the sphere that encloses everything (a light outside the skybox): upload the scene again."""
        flat = light_positions(lights)
        if isinstance(first, bool) or not isinstance(first, int) or first < 0:
            raise ValueError("first must be a light index")
        xyz = (C.c_double * max(len(flat), 1))(*flat)
        _check(self.lib, self.lib.rt_scene_set_lights(self.handle, first, len(flat) // 3, xyz, C.c_void_p(stream or 0)), "rt_scene_set_lights")

    def set_light_intensity(self, value):
        """The intensity all lights share (main.js:284) for the scene's later renders.  Host state only, like the stars seed: renders
        already enqueued keep theirs."""
        if isinstance(value, bool) or not isinstance(value, numbers.Real):
            raise ValueError("light intensity must be a number")
        _check(self.lib, self.lib.rt_scene_set_light_intensity(self.handle, float(value)), "rt_scene_set_light_intensity")

    def texture_size(self, texture):
        """(width, height) of texture `texture` of the resident scene, from the blob it was uploaded from (an edit never changes them)."""
        n_textures, = struct.unpack_from("<I", self.blob, 176)
        tex_off, = struct.unpack_from("<Q", self.blob, 200)
        if isinstance(texture, bool) or not isinstance(texture, int) or not 0 <= texture < n_textures:
            raise ValueError("texture must be an index below %d" % n_textures)
        return struct.unpack_from("<II", self.blob, tex_off + TEXDESC_BYTES * texture)

    def set_texels(self, texture, texels, x=0, y=0, width=None, height=None, pitch=0, stream=None):
        """Replace the texels of the rectangle [x, x + width) x [y, y + height) of texture `texture` of the resident scene (default: from
        (x, y) to the texture's right and bottom edge; with x = y = 0 the whole texture) with `texels`: bytes (height rows of `pitch`
        bytes, 0 = 4 * width; the last row may end with its texels) or a (height, width, 4) uint8 array.  HOST memory, free again when
        the call returns; enqueued on `stream` (None = the library's), ordered against the scene's renders on every stream: renders
        issued before keep the old texels, the next one sees the new ones, nothing waits.  ValueError, before any library call, for
        texels of the wrong size."""
        tw, th = self.texture_size(texture)
        for v in (x, y, pitch):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError("x, y and pitch must be non-negative integers")
        w = tw - x if width is None else width
        h = th - y if height is None else height
        for v in (w, h):
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError("the rectangle [%r, %r + %r) x [%r, %r + %r) is none of texture %d (%dx%d)" % (x, x, w, y, y, h, texture, tw, th))
        if hasattr(texels, "shape"):
            if tuple(texels.shape) != (h, w, 4) or str(texels.dtype) != "uint8" or pitch not in (0, 4 * w):
                raise ValueError("texels must be a (%d, %d, 4) uint8 array (got %r %s)" % (h, w, tuple(texels.shape), texels.dtype))
            data = texels.tobytes()
        elif isinstance(texels, (bytes, bytearray, memoryview)):
            data = bytes(texels)
        else:
            raise ValueError("texels must be bytes or a (height, width, 4) uint8 array")
        row = pitch or 4 * w
        if pitch and (pitch < 4 * w or pitch % 4):
            raise ValueError("pitch must be 0 or a multiple of 4 that is at least 4 * width")
        need = 0 if w == 0 or h == 0 else (h - 1) * row + 4 * w
        if len(data) != need and len(data) != h * row:
            raise ValueError("%d rows of %d texels at a pitch of %d bytes are %d bytes, got %d" % (h, w, row, need, len(data)))
        buf = C.create_string_buffer(data, max(len(data), 1))
        _check(self.lib, self.lib.rt_scene_set_texels(self.handle, texture, x, y, w, h, buf, pitch, C.c_void_p(stream or 0)), "rt_scene_set_texels")

    def set_texels_device(self, texture, src_ptr, x, y, width, height, pitch=0, stream=None):
        """The same from DEVICE memory (src_ptr: 4-byte aligned, `height` rows of `pitch` bytes, 0 = 4 * width): one copy kernel on
        `stream`, behind whatever wrote src_ptr there - a frame render_tiles has just put into it becomes the texture without leaving
        the GPU and without a host wait."""
        _check(self.lib, self.lib.rt_scene_set_texels_device(self.handle, texture, x, y, width, height, C.c_void_p(src_ptr or 0), pitch,
                                                             C.c_void_p(stream or 0)), "rt_scene_set_texels_device")

    def render_tiles(self, w, h, d_out, tiles=None, stream=None, flags=0, want_stats=False):
        t = tiles if isinstance(tiles, RtTiles) else RtTiles(*(tiles or (h, 0, 1, 1)))
        st = RtStats() if want_stats else None
        rc = self.lib.rt_render_tiles_device(self.handle, w, h, C.byref(t), C.c_void_p(d_out), C.c_void_p(stream or 0),
                                             flags, C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_render_tiles_device")
        return st

    def render_batch(self, w, h, d_out, tiles, n_frames, frame_stride_bytes, stream=None, flags=0, want_stats=False):
        """n_frames frames' worth of `tiles` in ONE launch; frame f lands at d_out + f*frame_stride_bytes."""
        t = tiles if isinstance(tiles, RtTiles) else RtTiles(*tiles)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_render_batch_device(self.handle, w, h, C.byref(t), n_frames, C.c_void_p(d_out), frame_stride_bytes,
                                             C.c_void_p(stream or 0), flags, C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_render_batch_device")
        return st

    def render_scatter(self, w, h, frame_ptrs, tiles, stream=None, flags=0, want_stats=False):
        """`tiles` of len(frame_ptrs) frames in ONE launch; frame f's rows go to their place in the whole RGBA8 frame at
        frame_ptrs[f] (which may be another GPU's memory, peer-mapped with rt_ipc_open)."""
        t = tiles if isinstance(tiles, RtTiles) else RtTiles(*tiles)
        st = RtStats() if want_stats else None
        arr = (C.c_void_p * len(frame_ptrs))(*frame_ptrs)
        rc = self.lib.rt_render_scatter_device(self.handle, w, h, C.byref(t), len(frame_ptrs), arr, C.c_void_p(stream or 0), flags,
                                               C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_render_scatter_device")
        return st

    def compact_count(self, w, h, tiles, stream=None):
        """(blocks, bytes per block) of a compact band (RT_FLAG_COMPACT) over `tiles` for the scene's current camera."""
        t = tiles if isinstance(tiles, RtTiles) else RtTiles(*tiles)
        n, bb = C.c_uint32(), C.c_uint32()
        _check(self.lib, self.lib.rt_compact_count(self.handle, w, h, C.byref(t), C.c_void_p(stream or 0), C.byref(n), C.byref(bb)), "rt_compact_count")
        return n.value, bb.value

    def compact_expand(self, w, h, tiles, d_compact, d_frame, stream=None):
        """Put the blocks of a compact band over `tiles` (rendered here or on a rank that holds the same scene and camera) back into the RGBA8 frame."""
        t = tiles if isinstance(tiles, RtTiles) else RtTiles(*tiles)
        _check(self.lib, self.lib.rt_compact_expand_device(self.handle, w, h, C.byref(t), C.c_void_p(d_compact), C.c_void_p(d_frame), C.c_void_p(stream or 0)), "rt_compact_expand_device")

    def render_hits(self, w, h, id_ptr, depth_ptr, normal_ptr, tiles=None, stream=None, want_stats=False):
        """Primary hits of `tiles` (output rows) into DEVICE buffers (0 / None = not wanted): per sample int32 id (sphere index |
        inside << 16, -1 = miss), float64 depth, 3 x float32 normal; tile slot i holds its k*tile_rows sample rows of k*w samples."""
        t = tiles if isinstance(tiles, RtTiles) else RtTiles(*(tiles or (h, 0, 1, 1)))
        bufs = RtHitBuffers(id_ptr or None, depth_ptr or None, normal_ptr or None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_render_hits_device(self.handle, w, h, C.byref(t), C.byref(bufs), C.c_void_p(stream or 0),
                                            C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_render_hits_device")
        return st

    def render_adaptive(self, w, h, d_out, k, threshold, work_ptr, work_bytes, mask_ptr=0, stream=None, flags=0, want_stats=False):
        """Adaptive supersampling of the whole w x h frame into DEVICE memory: the supersample-1 frame, then k x k samples (k 2..4) for
        the pixels that differ from a 4-neighbour by `threshold` (0..256) or more in R, G or B.  work_ptr: work_bytes >=
        adaptive_work_bytes(w, h) bytes of device workspace, whose first uint32 holds the number of refined pixels when the work is
        done; mask_ptr (0 / None = not wanted): w * h bytes, 1 = refined.  flags: 0 or RT_FLAG_STRICT_FP (the base launch's)."""
        st = RtStats() if want_stats else None
        rc = self.lib.rt_render_adaptive_device(self.handle, w, h, k, threshold, C.c_void_p(d_out or 0), C.c_void_p(mask_ptr or 0), C.c_void_p(work_ptr or 0),
                                                work_bytes, C.c_void_p(stream or 0), flags, C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_render_adaptive_device")
        return st

    def pick(self, w, h, points):
        """Hit records of sample points [(x, y), ...] (sample-grid coordinates), with the scene's current camera: a list of dicts
        (_hit_dict), None for a miss."""
        n, xy = _points_array(points)
        return _pick_call(self.lib, lambda n, xy, out: self.lib.rt_scene_pick(self.handle, w, h, n, xy, out), n, xy, "rt_scene_pick")

    def trace_rays(self, n, rays_ptr, rgb_ptr, rgba_ptr, hits_ptr, segs=0, stream=None, want_stats=False):
        """intersectWorld(segs, objects, org, dir) (main.js:216-336) for n rays {org[3], dir[3]} (float64, 16-byte aligned) in DEVICE
        memory, into DEVICE buffers (0 / None = not wanted): 3 float64 rgb, 4 uint8 rgba, one 80-byte RtHit per ray.  The direction is
        used as given; segs 0 = the scene's depth; the scene's camera plays no part."""
        out = RtRayOutputs(rgb_ptr or None, rgba_ptr or None, hits_ptr or None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_trace_rays_device(self.handle, n, C.c_void_p(rays_ptr or 0), segs, C.byref(out), C.c_void_p(stream or 0),
                                                 C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_trace_rays_device")
        return st

    def order_rays(self, n, rays_ptr, order_ptr, work_ptr, work_bytes, stream=None):
        """Bin n rays in DEVICE memory: order_ptr (n uint32, DEVICE) receives a permutation of 0..n-1 in which 64 consecutive entries
        are rays close in origin and direction (non-finite rays last); work_ptr is work_bytes >= rays_order_work_bytes(n) bytes of
        device workspace.  Asynchronous; reads nothing of the scene."""
        rc = self.lib.rt_scene_order_rays_device(self.handle, n, C.c_void_p(rays_ptr or 0), C.c_void_p(order_ptr or 0), C.c_void_p(work_ptr or 0),
                                                 work_bytes, C.c_void_p(stream or 0))
        _check(self.lib, rc, "rt_scene_order_rays_device")

    def trace_rays_ordered(self, n, rays_ptr, order_ptr, rgb_ptr, rgba_ptr, hits_ptr, segs=0, stream=None, want_stats=False):
        """trace_rays in the order of order_ptr (n uint32, DEVICE: order_rays' result or any permutation of the caller's): work-item j
        traces ray order[j] and writes its outputs at that ray's index, so the buffers hold what trace_rays puts there.  An entry >= n
        is skipped."""
        out = RtRayOutputs(rgb_ptr or None, rgba_ptr or None, hits_ptr or None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_trace_rays_ordered_device(self.handle, n, C.c_void_p(rays_ptr or 0), C.c_void_p(order_ptr or 0), segs, C.byref(out),
                                                         C.c_void_p(stream or 0), C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_trace_rays_ordered_device")
        return st

    def view_rays(self, view, w, h, rays_ptr, first_row=0, rows=None, stream=None):
        """Rows [first_row, first_row + rows) (default: to the last) of `view`'s w x h primary rays into rays_ptr (DEVICE, 16-byte
        aligned, rows * w records of six float64), generated on the GPU: the bits of rt_host.view_rays.  Asynchronous; reads nothing of
        the scene.  An EQUIRECT view's tables are DEVICE pointers here."""
        rows = h - first_row if rows is None else rows
        rc = self.lib.rt_view_rays_device(self.device, C.byref(view), w, h, first_row, rows, C.c_void_p(rays_ptr or 0), C.c_void_p(stream or 0))
        _check(self.lib, rc, "rt_view_rays_device")

    def trace_view(self, view, w, h, rgb_ptr, rgba_ptr, hits_ptr, work_ptr, work_bytes, segs=0, stream=None, want_stats=False):
        """intersectWorld for every ray of `view` at w x h, into DEVICE buffers in frame order (0 / None = not wanted; rgba is the w x h
        RGBA8 frame): the rays are generated on the GPU band by band into work_ptr (DEVICE, 16-byte aligned, work_bytes >= 48 w;
        view_work_bytes(w, h) is the size the library prefers) and traced as trace_rays traces them, ray y w + x with pix = y w + x.
        The scene's own camera plays no part.  An EQUIRECT view's tables are DEVICE pointers here."""
        out = RtRayOutputs(rgb_ptr or None, rgba_ptr or None, hits_ptr or None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_trace_view_device(self.handle, C.byref(view), w, h, segs, C.byref(out), C.c_void_p(work_ptr or 0), work_bytes,
                                                 C.c_void_p(stream or 0), C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_trace_view_device")
        return st

    def view_sample_rays(self, view, w, h, sample, rays_ptr, lens=None, table=0, first_row=0, rows=None, stream=None):
        """view_rays for ONE sample (an RtViewSample: sub-pixel offset and lens point) and an optional lens: the bits of
        rt_host.view_sample_rays.  `table` is the index of the panorama table to read (EQUIRECT: DEVICE tables of several samples back to
        back, equirect_sample_tables' layout).  Asynchronous; reads nothing of the scene."""
        rows = h - first_row if rows is None else rows
        rc = self.lib.rt_view_sample_rays_device(self.device, C.byref(view), w, h, C.byref(lens) if lens is not None else None, C.byref(sample), table,
                                                 first_row, rows, C.c_void_p(rays_ptr or 0), C.c_void_p(stream or 0))
        _check(self.lib, rc, "rt_view_sample_rays_device")

    def trace_view_samples(self, view, w, h, samples, lens, rgb_ptr, rgba_ptr, work_ptr, work_bytes, segs=0, stream=None, want_stats=False):
        """The mean of n = len(samples) traces of `view` at w x h, one per sample (view_samples_grid(k), or the caller's own pattern),
        into DEVICE buffers in frame order (0 / None = not wanted): rgb the binary64 mean acc / n of the samples added in order, rgba
        that mean through the store rule.  lens: None or lens(radius, focus) (PINHOLE only).  Rays, one sample's rgb and the accumulator
        of a band live in work_ptr (DEVICE, 16-byte aligned, work_bytes >= 96 w; view_samples_work_bytes(w, h) is the size the library
        prefers).  Sample s draws its stars with pix = s w h + y w + x.  An EQUIRECT view's tables are DEVICE pointers to one table per
        sample (equirect_sample_tables)."""
        arr, n = _samples_array(samples)
        out = RtRayOutputs(rgb_ptr or None, rgba_ptr or None, None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_trace_view_samples_device(self.handle, C.byref(view), w, h, C.byref(lens) if lens is not None else None, n, arr, segs,
                                                         C.byref(out), C.c_void_p(work_ptr or 0), work_bytes, C.c_void_p(stream or 0),
                                                         C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_trace_view_samples_device")
        return st

    def occlusion(self, n, rays_ptr, length_ptr, intensity_ptr, skip_ptr, out_intensity_ptr, out_blocker_ptr, order_ptr=0, stream=None, want_stats=False):
        """The reference's shadow scan (main.js:293-304) for n segments {org[3], dir[3]} (float64, 16-byte aligned) in DEVICE memory: per
        ray the light intensity that is left (float64) and the opaque sphere that ended the scan (int32, -1 = none), into DEVICE buffers
        (0 / None = not wanted).  Inputs per ray, DEVICE, 0 / None = the default: float64 length (+Infinity), float64 intensity (the
        scene's), int32 skip (no sphere left out).  order_ptr: 0, or n uint32 (DEVICE) as trace_rays_ordered takes them."""
        ins = RtOcclusionInputs(length_ptr or None, intensity_ptr or None, skip_ptr or None)
        out = RtOcclusionOutputs(out_intensity_ptr or None, out_blocker_ptr or None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_occlusion_device(self.handle, n, C.c_void_p(rays_ptr or 0), C.c_void_p(order_ptr or 0), C.byref(ins), C.byref(out),
                                                C.c_void_p(stream or 0), C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_occlusion_device")
        return st

    def ambient_segments(self, n, hits_ptr, dirs_ptr, n_dirs, sample, rays_ptr, skip_ptr=0, n_samples=None, stride=1, base=0, stream=None):
        """The segments of sample `sample` of n receivers (HIT_DTYPE records, DEVICE, 8-byte aligned) into rays_ptr (DEVICE, 16-byte
        aligned, n records of six float64) and skip_ptr (DEVICE, n int32; 0 = not wanted), generated on the GPU: the bits of
        rt_host.ambient_segments.  dirs_ptr: n_dirs local directions (DEVICE, 3 float64 each).  What comes out goes into occlusion
        (length = the radius, intensity = 1.0, skip), order_rays or trace_rays as it is.  Asynchronous; reads nothing of the scene."""
        a = RtAmbient(sample + 1 if n_samples is None else n_samples, n_dirs, stride, 0, base, 1.0)
        rc = self.lib.rt_ambient_segments_device(self.device, C.byref(a), C.c_void_p(dirs_ptr or 0), n, C.c_void_p(hits_ptr or 0), sample,
                                                 C.c_void_p(rays_ptr or 0), C.c_void_p(skip_ptr or 0), C.c_void_p(stream or 0))
        _check(self.lib, rc, "rt_ambient_segments_device")

    def ambient(self, n, hits_ptr, dirs_ptr, n_dirs, n_samples, radius, open_ptr, intensity_ptr, rgba_ptr, stride=1, base=0, order_ptr=0, stream=None,
                want_stats=False):
        """Ambient occlusion of n receivers (HIT_DTYPE records, DEVICE) in one fused kernel: n_samples scans of length `radius` per
        receiver over the hemisphere of its facing normal, along the directions of the table dirs_ptr (DEVICE, n_dirs entries) - per
        receiver float64 open (the share of scans no opaque sphere ended), float64 intensity (their mean intensity, starting from 1.0)
        and uint32 rgba (open as a grey RGBA8 pixel) into DEVICE buffers (0 / None = not wanted).  order_ptr as occlusion takes it."""
        a = RtAmbient(n_samples, n_dirs, stride, 0, base, float(radius))
        out = RtAmbientOutputs(open_ptr or None, intensity_ptr or None, rgba_ptr or None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_ambient_device(self.handle, C.byref(a), C.c_void_p(dirs_ptr or 0), n, C.c_void_p(hits_ptr or 0), C.c_void_p(order_ptr or 0),
                                              C.byref(out), C.c_void_p(stream or 0), C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_ambient_device")
        return st

    def ambient_view(self, view, w, h, dirs_ptr, n_dirs, n_samples, radius, open_ptr, intensity_ptr, rgba_ptr, work_ptr, work_bytes, stride=1, base=0,
                     stream=None, want_stats=False):
        """ambient() for what `view` sees at w x h, pixel y w + x being receiver y w + x, into DEVICE buffers in frame order: rays, hit
        records and scans stay on the GPU, band by band in work_ptr (DEVICE, 16-byte aligned, work_bytes >= 128 w;
        ambient_view_work_bytes(w, h) is the size the library prefers).  An EQUIRECT view's tables are DEVICE pointers here."""
        a = RtAmbient(n_samples, n_dirs, stride, 0, base, float(radius))
        out = RtAmbientOutputs(open_ptr or None, intensity_ptr or None, rgba_ptr or None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_ambient_view_device(self.handle, C.byref(view), w, h, C.byref(a), C.c_void_p(dirs_ptr or 0), C.byref(out),
                                                   C.c_void_p(work_ptr or 0), work_bytes, C.c_void_p(stream or 0), C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_ambient_view_device")
        return st

    def lighting(self, n, hits_ptr, offs_ptr, n_offs, n_samples, light_radius, diffuse_ptr, intensity_ptr, lit_ptr, rgba_ptr, stride=1, base=0, order_ptr=0,
                 stream=None, want_stats=False):
        """The reference's light loop (main.js:283-306) for n receivers (HIT_DTYPE records, DEVICE) in one fused kernel, n_samples times
        with every light displaced by an entry of the table offs_ptr (DEVICE, n_offs entries of 3 float64; 0 where light_radius is 0)
        times light_radius, with the scene's CURRENT lights and light intensity - per receiver float64 diffuse (the mean raw diffuse sum),
        float64 intensity (the mean intensity left after the last light), float64 lit (the share of (sample, light) pairs that
        contributed) and uint32 rgba (min(1, diffuse) as a grey RGBA8 pixel) into DEVICE buffers (0 / None = not wanted).  order_ptr as
        occlusion takes it."""
        a = RtLighting(n_samples, n_offs, stride, 0, base, float(light_radius))
        out = RtLightingOutputs(diffuse_ptr or None, intensity_ptr or None, lit_ptr or None, rgba_ptr or None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_lighting_device(self.handle, C.byref(a), C.c_void_p(offs_ptr or 0), n, C.c_void_p(hits_ptr or 0), C.c_void_p(order_ptr or 0),
                                               C.byref(out), C.c_void_p(stream or 0), C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_lighting_device")
        return st

    def lighting_view(self, view, w, h, offs_ptr, n_offs, n_samples, light_radius, diffuse_ptr, intensity_ptr, lit_ptr, rgba_ptr, work_ptr, work_bytes,
                      stride=1, base=0, stream=None, want_stats=False):
        """lighting() for what `view` sees at w x h, pixel y w + x being receiver y w + x, into DEVICE buffers in frame order: rays, hit
        records and scans stay on the GPU, band by band in work_ptr (DEVICE, 16-byte aligned, work_bytes >= 128 w;
        lighting_view_work_bytes(w, h) is the size the library prefers).  An EQUIRECT view's tables are DEVICE pointers here."""
        a = RtLighting(n_samples, n_offs, stride, 0, base, float(light_radius))
        out = RtLightingOutputs(diffuse_ptr or None, intensity_ptr or None, lit_ptr or None, rgba_ptr or None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_lighting_view_device(self.handle, C.byref(view), w, h, C.byref(a), C.c_void_p(offs_ptr or 0), C.byref(out),
                                                    C.c_void_p(work_ptr or 0), work_bytes, C.c_void_p(stream or 0), C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_lighting_view_device")
        return st

    def shade_rays(self, n, rays_ptr, nodes_ptr, order_ptr=0, pix_ptr=0, path_ptr=0, stream=None, want_stats=False):
        """One level of intersectWorld (main.js:216-336 without its two recursive calls) for n rays in DEVICE memory: node i (NODE_DTYPE,
        200 bytes, 8-byte aligned) per ray i into nodes_ptr (DEVICE).  order_ptr as trace_rays_ordered takes it; pix_ptr / path_ptr: n uint32
        each (DEVICE), the stars sampler's pix and path per ray, 0 / None = i and 1."""
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_shade_rays_device(self.handle, n, C.c_void_p(rays_ptr or 0), C.c_void_p(order_ptr or 0), C.c_void_p(pix_ptr or 0),
                                                 C.c_void_p(path_ptr or 0), C.c_void_p(nodes_ptr or 0), C.c_void_p(stream or 0),
                                                 C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_shade_rays_device")
        return st

    def relight_nodes(self, n, rays_ptr, nodes_ptr, offs_ptr, n_offs, n_samples, light_radius, stride=1, base=0, order_ptr=0, pix_ptr=0, stream=None,
                      want_stats=False):
        """Soft lights for n shaded nodes (DEVICE, what shade_rays wrote for the n rays at rays_ptr): the node's diffuse and specular terms
        computed again n_samples times with every light displaced by light_radius times an entry of the table offs_ptr (DEVICE, n_offs
        entries of 3 float64; 0 where light_radius is 0), clamped and weighted per sample, and their means written back into the node
        (bytes 104..119; nothing else).  Sample s of node i uses entry ((base + pix_i) stride + s) % n_offs, pix_i = pix_ptr[i] (n uint32,
        DEVICE) or i.  order_ptr as shade_rays takes it.  With the scene's CURRENT lights, light intensity and spheres."""
        a = RtLighting(n_samples, n_offs, stride, 0, base, float(light_radius))
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_relight_nodes_device(self.handle, C.byref(a), C.c_void_p(offs_ptr or 0), n, C.c_void_p(rays_ptr or 0), C.c_void_p(order_ptr or 0),
                                                    C.c_void_p(pix_ptr or 0), C.c_void_p(nodes_ptr or 0), C.c_void_p(stream or 0),
                                                    C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_relight_nodes_device")
        return st

    def trace_rays_soft(self, n, rays_ptr, rgb_ptr, rgba_ptr, offs_ptr, n_offs, n_samples, light_radius, stride=1, base=0, levels=1, segs=0, order_ptr=0,
                        pix_base=0, stream=None, want_stats=False):
        """The soft trace in ONE launch: intersectWorld for n rays in DEVICE memory, walked depth-first over a per-lane stack, with the
        light terms of the nodes at tree levels below `levels` sampled as relight_nodes samples them - rt_host.trace_rays_soft's rgb
        (3 float64 per ray) and rgba into DEVICE buffers (0 / None = not wanted), bit for bit, without nodes in device memory and without
        a host wait.  Sample s of every node of ray i uses entry ((base + pix_base + i) stride + s) % n_offs of the table offs_ptr (DEVICE;
        0 where light_radius is 0); pix_base is the index of the list's first ray in the caller's whole list (the stars sampler's pix is
        pix_base + i too), so a list traced in pieces gives the bytes of one call.  order_ptr as trace_rays_ordered takes it.  With the
        scene's CURRENT lights, light intensity and spheres."""
        a = RtLighting(n_samples, n_offs, stride, 0, base, float(light_radius))
        out = RtRayOutputs(rgb_ptr or None, rgba_ptr or None, None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_trace_rays_soft_device(self.handle, C.byref(a), C.c_void_p(offs_ptr or 0), levels, n, C.c_void_p(rays_ptr or 0),
                                                      C.c_void_p(order_ptr or 0), pix_base, segs, C.byref(out), C.c_void_p(stream or 0),
                                                      C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_trace_rays_soft_device")
        return st

    def trace_view_soft(self, view, w, h, rgb_ptr, rgba_ptr, offs_ptr, n_offs, n_samples, light_radius, work_ptr, work_bytes, stride=1, base=0, levels=1,
                        segs=0, stream=None, want_stats=False):
        """trace_rays_soft() for what `view` sees at w x h, pixel y w + x being ray y w + x, into DEVICE buffers in frame order: the rays
        are generated on the GPU band by band in work_ptr (DEVICE, 16-byte aligned, work_bytes >= 48 w; soft_view_work_bytes(w, h) is the
        size the library prefers) and each band is one launch.  An EQUIRECT view's tables are DEVICE pointers here."""
        a = RtLighting(n_samples, n_offs, stride, 0, base, float(light_radius))
        out = RtRayOutputs(rgb_ptr or None, rgba_ptr or None, None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_trace_view_soft_device(self.handle, C.byref(view), w, h, C.byref(a), C.c_void_p(offs_ptr or 0), levels, segs, C.byref(out),
                                                      C.c_void_p(work_ptr or 0), work_bytes, C.c_void_p(stream or 0), C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_trace_view_soft_device")
        return st

    def gather(self, n, hits_ptr, dirs_ptr, n_dirs, n_samples, rgb_ptr, rgba_ptr, stride=1, segs=0, base=0, pix_base=0, pix_stride=None, order_ptr=0,
               stream=None, want_stats=False):
        """Gathered light of n receivers (HIT_DTYPE records, DEVICE) in ONE fused kernel: per receiver n_samples rays leave the point along
        the directions ambient_segments defines (table dirs_ptr: DEVICE, n_dirs entries), each traced as trace_rays traces any ray (depth
        `segs`, 0 = the scene's; no sphere left out) with the scene's CURRENT spheres, lights, textures and stars seed, and their mean
        goes into rgb_ptr (3 float64 per receiver) and rgba_ptr (uint32, the store rule) - DEVICE buffers, 0 / None = not wanted.  No
        segment and no per-sample colour exists in memory.  The stars sampler's pix of sample s of receiver i is
        pix_base + s pix_stride + i (pix_stride None = n).  order_ptr as ambient takes it."""
        a = RtGather(n_samples, n_dirs, stride, segs, base, pix_base, n if pix_stride is None else pix_stride)
        out = RtGatherOutputs(rgb_ptr or None, rgba_ptr or None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_gather_device(self.handle, C.byref(a), C.c_void_p(dirs_ptr or 0), n, C.c_void_p(hits_ptr or 0), C.c_void_p(order_ptr or 0),
                                             C.byref(out), C.c_void_p(stream or 0), C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_gather_device")
        return st

    def gather_probes(self, n, hits_ptr, dirs_ptr, n_dirs, n_samples, rgb_ptr, rgba_ptr, coef_ptr=0, weights_ptr=0, n_weights=0, stride=1, segs=0, base=0,
                      pix_base=0, pix_stride=None, order_ptr=0, stream=None, want_stats=False):
        """gather() for a SHORT list (light probes): one workgroup per receiver with its samples on lanes; rgb_ptr and rgba_ptr receive
        gather's bytes.  With weights_ptr (DEVICE, n_dirs rows of n_weights float64, 1..16) coef_ptr (DEVICE, n x n_weights x 3 float64)
        receives per receiver, weight k and channel the mean of w[e_s][k] c_s, e_s being the table entry sample s took its direction
        from - with sh9_weights of a sphere table, the probe's nine spherical-harmonics coefficients up to the factor 4 pi.  Everything
        else as gather()."""
        a = RtGather(n_samples, n_dirs, stride, segs, base, pix_base, n if pix_stride is None else pix_stride)
        out = RtProbeOutputs(rgb_ptr or None, rgba_ptr or None, coef_ptr or None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_gather_probes_device(self.handle, C.byref(a), C.c_void_p(dirs_ptr or 0), C.c_void_p(weights_ptr or 0), n_weights, n,
                                                    C.c_void_p(hits_ptr or 0), C.c_void_p(order_ptr or 0), C.byref(out), C.c_void_p(stream or 0),
                                                    C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_gather_probes_device")
        return st

    def gather_view(self, view, w, h, dirs_ptr, n_dirs, n_samples, rgb_ptr, rgba_ptr, work_ptr, work_bytes, stride=1, segs=0, base=0, pix_base=0,
                    pix_stride=None, stream=None, want_stats=False):
        """gather() for what `view` sees at w x h, pixel y w + x being receiver y w + x, into DEVICE buffers in frame order: rays, hit
        records and the gathered rays stay on the GPU, band by band in work_ptr (DEVICE, 16-byte aligned, work_bytes >= 128 w;
        gather_view_work_bytes(w, h) is the size the library prefers).  pix_stride None = w h, the sampled view's pix = s w h + y w + x.
        An EQUIRECT view's tables are DEVICE pointers here."""
        a = RtGather(n_samples, n_dirs, stride, segs, base, pix_base, w * h if pix_stride is None else pix_stride)
        out = RtGatherOutputs(rgb_ptr or None, rgba_ptr or None)
        st = RtStats() if want_stats else None
        rc = self.lib.rt_scene_gather_view_device(self.handle, C.byref(view), w, h, C.byref(a), C.c_void_p(dirs_ptr or 0), C.byref(out),
                                                  C.c_void_p(work_ptr or 0), work_bytes, C.c_void_p(stream or 0), C.byref(st) if st is not None else None)
        _check(self.lib, rc, "rt_scene_gather_view_device")
        return st

    def spawn_rays(self, n, nodes_ptr, child_rays_ptr, links_ptr, count_ptr, work_ptr, work_bytes, pix_ptr=0, path_ptr=0, child_pix_ptr=0,
                   child_path_ptr=0, stream=None):
        """The children of n nodes (DEVICE) as the next level's ray list: child_rays_ptr (2n x 6 float64), child_pix_ptr / child_path_ptr
        (2n uint32 each, 0 = not wanted), links_ptr (2n int32: per parent its reflect and refract child's index, or -1), count_ptr (one
        uint32), all DEVICE; stable, by parent, reflect before refract.  work_ptr: work_bytes >= nodes_spawn_work_bytes(n) of device
        workspace.  Asynchronous, no host wait."""
        rc = self.lib.rt_scene_spawn_rays_device(self.handle, n, C.c_void_p(nodes_ptr or 0), C.c_void_p(pix_ptr or 0), C.c_void_p(path_ptr or 0),
                                                 C.c_void_p(child_rays_ptr or 0), C.c_void_p(child_pix_ptr or 0), C.c_void_p(child_path_ptr or 0),
                                                 C.c_void_p(links_ptr or 0), C.c_void_p(count_ptr or 0), C.c_void_p(work_ptr or 0), work_bytes,
                                                 C.c_void_p(stream or 0))
        _check(self.lib, rc, "rt_scene_spawn_rays_device")

    def fold_nodes(self, n, nodes_ptr, links_ptr, child_rgb_ptr, rgb_ptr, rgba_ptr, stream=None):
        """main.js:322-336 for n nodes (DEVICE): the children's colours (child_rgb_ptr, 3 float64 each) gathered through links_ptr (0 = the
        deepest level: every child is [0, 0, 0]) into rgb_ptr (3 float64 per node) and / or rgba_ptr (4 uint8), DEVICE, 0 = not wanted."""
        rc = self.lib.rt_scene_fold_nodes_device(self.handle, n, C.c_void_p(nodes_ptr or 0), C.c_void_p(links_ptr or 0), C.c_void_p(child_rgb_ptr or 0),
                                                 C.c_void_p(rgb_ptr or 0), C.c_void_p(rgba_ptr or 0), C.c_void_p(stream or 0))
        _check(self.lib, rc, "rt_scene_fold_nodes_device")

    def close(self):
        if self.handle:
            self.lib.rt_scene_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build_id(lib=None):
    """`const build = '741'` (main.js:3) + the library's revision, e.g. '741.r4'."""
    return (lib or load_library()).rt_build_id().decode()


def elapsed_report(stats, lib=None):
    """The reference's end-of-frame string for a finished render (main.js:204-205): 'build #<id> (<elapsed>ms)'."""
    lib = lib or load_library()
    buf = C.create_string_buffer(96)
    n = lib.rt_elapsed_report(C.byref(stats), buf, len(buf))
    if n < 0:
        raise RtError("rt_elapsed_report failed: " + lib.rt_last_error().decode())
    return buf.value.decode()


def render(width, height, scene, flags=0, lib=None, max_devices=1):
    """render(width,height,scene) -> (bytes RGBA8, RtStats): the whole-frame entry point, host buffer out.
    max_devices > 1 (or 0 = all) lets rt_render shard the frame over the node's GPUs (RCCL gather)."""
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    _check(lib, lib.rt_init(max_devices), "rt_init")
    n = width * height * 4
    p = lib.rt_alloc_pinned(n)
    if not p:
        raise RtError("rt_alloc_pinned(%d) failed: %s" % (n, lib.rt_last_error().decode()))
    try:
        st = RtStats()
        buf = C.create_string_buffer(blob, len(blob))
        _check(lib, lib.rt_render(buf, len(blob), width, height, C.c_void_p(p), flags, C.byref(st)), "rt_render")
        return C.string_at(p, n), st
    finally:
        lib.rt_free_pinned(p)


def _init_once(lib):
    if lib.rt_device_count() < 0:                     # not initialised yet: one GPU, as render() (an earlier rt_init's choice stands)
        _check(lib, lib.rt_init(1), "rt_init")


def _hit_dict(r):
    if r.object < 0:
        return None
    return {"object": r.object, "inside": bool(r.inside), "t": r.t, "point": list(r.point), "normal": list(r.normal), "u": r.u, "v": r.v}


def _points_array(points):
    pts = [(int(x), int(y)) for x, y in points]
    if not all(0 <= c < 2 ** 32 for p in pts for c in p):
        raise ValueError("sample coordinates must be integers in [0, 2^32)")
    return len(pts), (C.c_uint32 * (2 * len(pts)))(*[c for p in pts for c in p])


def _pick_call(lib, call, n, xy, what):
    if n == 0:
        return []
    out = (RtHit * n)()
    _check(lib, call(n, xy, out), what)
    return [_hit_dict(r) for r in out]


def hits(width, height, scene, lib=None):
    """hits(width,height,scene) -> {"id": int32 (kh, kw), "depth": float64 (kh, kw), "normal": float32 (kh, kw, 3)}: the primary hit of
    every sample (k = the scene's supersample factor), rendered on GPU 0 with rt_render's resident scene."""
    import numpy as np
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    k = struct.unpack_from("<I", blob, 164)[0]          # rt_scene_header.supersample
    _init_once(lib)
    out = {"id": np.empty((k * height, k * width), np.int32), "depth": np.empty((k * height, k * width), np.float64),
           "normal": np.empty((k * height, k * width, 3), np.float32)}
    bufs = RtHitBuffers(out["id"].ctypes.data, out["depth"].ctypes.data, out["normal"].ctypes.data)
    buf = C.create_string_buffer(blob, len(blob))
    _check(lib, lib.rt_render_hits(buf, len(blob), width, height, C.byref(bufs), None), "rt_render_hits")
    return out


def pick(width, height, scene, points, lib=None):
    """pick(width,height,scene,points) -> [hit dict or None per (x, y) sample point] on GPU 0 with rt_render's resident scene."""
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    n, xy = _points_array(points)
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    return _pick_call(lib, lambda n, xy, out: lib.rt_pick(buf, len(blob), width, height, n, xy, out), n, xy, "rt_pick")


def adaptive_work_bytes(w, h, lib=None):
    """Bytes of device workspace Renderer.render_adaptive needs for a w x h frame (host arithmetic: 16 + 4 w h; 0 for an empty frame or a
    side above 32768)."""
    return int((lib or load_library()).rt_adaptive_work_bytes(w, h))


def render_adaptive(width, height, scene, k=4, threshold=32, want_mask=False, flags=0, lib=None):
    """render_adaptive(width,height,scene) -> (bytes RGBA8, RtStats, refined pixels[, mask bytes]): the supersample-1 frame with k x k
    samples where it has edges (Renderer.render_adaptive), on GPU 0 with rt_render's resident scene, host buffers out."""
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    _init_once(lib)
    out = C.create_string_buffer(width * height * 4)
    mask = C.create_string_buffer(width * height) if want_mask else None
    st, refined = RtStats(), C.c_uint64()
    buf = C.create_string_buffer(blob, len(blob))
    _check(lib, lib.rt_render_adaptive(buf, len(blob), width, height, k, threshold, out, mask, flags, C.byref(st), C.byref(refined)), "rt_render_adaptive")
    res = (out.raw, st, int(refined.value))
    return res + (mask.raw,) if want_mask else res


def adaptive_mask(frame, w, h, threshold):
    """The criterion of adaptive supersampling in numpy: an (h, w) uint8 array, 1 where the pixel of the RGBA8 `frame` (bytes or array)
    has a 4-neighbour inside the frame that differs from it by at least `threshold` in R, G or B (integers; alpha plays no part).
    threshold 0 marks every pixel - a 1 x 1 frame's too -, 256 none."""
    import numpy as np
    f = np.frombuffer(frame, np.uint8) if isinstance(frame, (bytes, bytearray, memoryview)) else np.asarray(frame, np.uint8)
    f = f.reshape(h, w, 4)[..., :3].astype(np.int32)
    m = np.zeros((h, w), np.int32)                        # the largest difference to a neighbour; no neighbour: 0
    dx = np.abs(f[:, 1:] - f[:, :-1]).max(axis=2)
    dy = np.abs(f[1:, :] - f[:-1, :]).max(axis=2)
    m[:, 1:] = np.maximum(m[:, 1:], dx); m[:, :-1] = np.maximum(m[:, :-1], dx)
    m[1:, :] = np.maximum(m[1:, :], dy); m[:-1, :] = np.maximum(m[:-1, :], dy)
    return (m >= int(threshold)).astype(np.uint8)


def adaptive_compose(base, fine, mask):
    """The adaptive frame from its parts: `fine`'s pixel where `mask` is set, `base`'s elsewhere.  base, fine: RGBA8 frames of one size
    (bytes or arrays); mask: (h, w).  Returns an (h, w, 4) uint8 array."""
    import numpy as np
    m = np.asarray(mask).astype(bool)
    h, w = m.shape
    b = (np.frombuffer(base, np.uint8) if isinstance(base, (bytes, bytearray, memoryview)) else np.asarray(base, np.uint8)).reshape(h, w, 4)
    f = (np.frombuffer(fine, np.uint8) if isinstance(fine, (bytes, bytearray, memoryview)) else np.asarray(fine, np.uint8)).reshape(h, w, 4)
    return np.where(m[..., None], f, b)


def normal3d(v):
    """The reference's normal3D (main.js:62-66) on an (..., 3) float64 array: multiply by 1 / sqrt(x x + y y + z z); a zero vector is
    returned unchanged.  trace_rays uses directions as given - this is what the reference applies before it calls intersectWorld."""
    import numpy as np
    v = np.asarray(v, np.float64)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    l = np.sqrt(x * x + y * y + z * z)
    with np.errstate(divide="ignore"):
        k = np.where(l != 0.0, 1.0 / l, 1.0)
    return np.where((l != 0.0)[..., None], v * k[..., None], v)


def primary_rays(width, height, scene):
    """The primary rays of the width x height frame (main.js:184-193, operation for operation in binary64: dist indexed by component -
    quirk q1 -, the additions in the reference's order, between3D, normal3D with its l != 0 guard) as a (k width * k height, 6) float64
    array {org, dir} in row order of the k width x k height sample grid (k = the scene's supersample factor).  trace_rays of this list
    is the scene's RT_FLAG_STRICT_FP sample frame, stars included (a ray's index in the list is its sample's index in the frame)."""
    import math
    import numpy as np
    cam = scene["camera"]
    k = scene.get("supersample", 1)
    sw, sh = k * width, k * height
    proj_w, proj_h = float(width) * k / 2.0, float(height) * k / 2.0
    proj_d = proj_w / math.tan(float(scene.get("fovDeg", 60)) * math.pi / 180.0 / 2.0)
    o, ax, ay, az = (np.array(cam[n], np.float64) for n in ("origin", "axisX", "axisY", "axisZ"))
    d0 = np.broadcast_to((np.arange(sw, dtype=np.float64) - proj_w) + 0.5, (sh, sw))
    d1 = np.broadcast_to(((proj_h - np.arange(sh, dtype=np.float64)) - 0.5)[:, None], (sh, sw))
    d2 = np.full((sh, sw), proj_d)
    rays = np.empty((sh, sw, 6), np.float64)
    for c, d in enumerate((d0, d1, d2)):
        target = o[c] + ax[c] * d + ay[c] * d + az[c] * d
        rays[..., c] = o[c]
        rays[..., 3 + c] = target - o[c]
    rays[..., 3:] = normal3d(rays[..., 3:])
    return rays.reshape(sh * sw, 6)


def rays_order_work_bytes(n, lib=None):
    """Bytes of device workspace Renderer.order_rays needs for n rays (host arithmetic; 0 for n == 0 and n >= 2^31)."""
    return int((lib or load_library()).rt_rays_order_work_bytes(n))


def trace_rays(scene, rays, segs=0, want=("rgb",), lib=None, order="list", method="recursive", order_levels=False):
    """trace_rays(scene, rays) -> {"rgb": (n, 3) float64, "rgba": (n, 4) uint8, "hits": [hit dict or None per ray]} (the keys named in
    `want`): intersectWorld(segs, objects, org, dir) per row {org, dir} of the float64 (n, 6) array `rays`, directions as given, on
    GPU 0 with rt_render's resident scene.  segs 0 = the scene's depth.  A ray with a non-finite component is not traced: NaN, NaN,
    NaN / 0, 0, 0, 255 / None.  order: "list" traces the rays in the list's order; "binned" (rt_trace_rays_binned) has the GPU put
    each chunk of 2^18 rays into an order in which neighbours are neighbours in space first - the same results, sooner for a list
    that is not coherent.  method: "recursive" (the one kernel that runs the whole ray tree), or "wavefront" (rt_trace_rays_wavefront:
    level by level through shade, spawn and fold - the same bytes in rgb and rgba; no hits; order "list" only; order_levels=True bins
    every level after the first before it is shaded; `want` may name "level_counts": uint64[16], the rays shaded per level)."""
    import numpy as np
    if order not in ("list", "binned"):
        raise ValueError("order is 'list' or 'binned'")
    if method not in ("recursive", "wavefront"):
        raise ValueError("method is 'recursive' or 'wavefront'")
    wavefront = method == "wavefront"
    if wavefront and order != "list":
        raise ValueError("method 'wavefront' takes the first level in the list's order (order_levels bins the others)")
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    want = set(want)
    allowed = {"rgb", "rgba", "level_counts"} if wavefront else {"rgb", "rgba", "hits"}
    if not (want - {"level_counts"}) or want - allowed:
        raise ValueError("want names some of %s" % ", ".join(repr(k) for k in sorted(allowed)))
    rays = np.asarray(rays, np.float64)
    if rays.ndim != 2 or rays.shape[1] != 6:
        raise ValueError("rays must be an (n, 6) array: org[3], dir[3] per row")
    n = rays.shape[0]
    aligned = np.empty(n * 6 + 2, np.float64)             # a contiguous copy on a 16-byte boundary
    aligned = aligned[(aligned.ctypes.data >> 3) & 1:][:n * 6]
    aligned[:] = rays.reshape(-1)
    out = {}
    if "rgb" in want:
        out["rgb"] = np.empty((n, 3), np.float64)
    if "rgba" in want:
        out["rgba"] = np.empty((n, 4), np.uint8)
    records = (RtHit * max(n, 1))() if "hits" in want else None
    bufs = RtRayOutputs(out["rgb"].ctypes.data if "rgb" in out else None, out["rgba"].ctypes.data if "rgba" in out else None,
                        C.addressof(records) if records is not None else None)
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    if wavefront:
        counts = np.zeros(RT_MAX_SEGS, np.uint64)
        rc = lib.rt_trace_rays_wavefront(buf, len(blob), n, C.c_void_p(aligned.ctypes.data), segs, 1 if order_levels else 0, C.byref(bufs), None,
                                         counts.ctypes.data_as(C.POINTER(C.c_uint64)))
        _check(lib, rc, "rt_trace_rays_wavefront")
        if "level_counts" in want:
            out["level_counts"] = counts
        return out
    call, what = (lib.rt_trace_rays, "rt_trace_rays") if order == "list" else (lib.rt_trace_rays_binned, "rt_trace_rays_binned")
    _check(lib, call(buf, len(blob), n, C.c_void_p(aligned.ctypes.data), segs, C.byref(bufs), None), what)
    if records is not None:
        out["hits"] = [_hit_dict(r) for r in records[:n]]
    return out


# --------------------------------------------------------------------------- views: a camera's rays generated on the GPU
def _aligned_f64(n):
    """n float64 on a 16-byte boundary."""
    import numpy as np
    a = np.empty(n + 2, np.float64)
    return a[(a.ctypes.data >> 3) & 1:][:n]


def view(model, origin, axis_x, axis_y, axis_z, fov_deg=60, scale=1.0, tables=None):
    """-> RtView.  model: RT_VIEW_REFERENCE (the reference's own per-component rays, main.js:186-193: a pinhole only while the axes
    are the world's), RT_VIEW_PINHOLE (a true pinhole for any basis), RT_VIEW_ORTHO (parallel rays along axis_z, `scale` world units per
    pixel) or RT_VIEW_EQUIRECT (a panorama; tables = equirect_tables(w, h) for the host forms, or a pair of DEVICE pointers for the
    Renderer's).  The axes are used as given: image x runs along axis_x, image y (upwards) along axis_y, the view looks along axis_z."""
    v = RtView()
    v.model, v.reserved = model, 0
    v.origin[:] = [float(x) for x in origin]
    v.axis_x[:] = [float(x) for x in axis_x]
    v.axis_y[:] = [float(x) for x in axis_y]
    v.axis_z[:] = [float(x) for x in axis_z]
    v.fov_deg, v.scale = float(fov_deg), float(scale)
    if tables is not None:
        lon, lat = tables
        if isinstance(lon, numbers.Integral):
            v.lon, v.lat = lon or None, lat or None
        else:
            v.lon, v.lat = lon.ctypes.data, lat.ctypes.data
            v._tables = (lon, lat)                       # (kept alive with the view)
    return v


def _copy_view(v):
    c = RtView.from_buffer_copy(bytes(v))
    if hasattr(v, "_tables"):
        c._tables = v._tables
    return c


def look_at_view(model, org, tgt, up, fov_deg=60, scale=1.0, tables=None):
    """view() with the basis of the reference's lookAt (main.js:92-100): axis_z = unit(tgt - org), axis_x = unit(cross(up, tgt - org)),
    axis_y = unit(cross(tgt - org, cross(up, tgt - org))).  Note that this axis_x points to the LEFT of the viewer (the reference's
    pictures are drawn that way round); negate it for an image whose x runs to the right."""
    import numpy as np

    def cross(a, b):
        return np.array([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]])
    org, tgt, up = (np.array(x, np.float64) for x in (org, tgt, up))
    z = tgt - org
    x = cross(up, z)
    y = cross(z, x)
    return view(model, org, normal3d(x), normal3d(y), normal3d(z), fov_deg, scale, tables)


def cube_views(eye):
    """Six RT_VIEW_PINHOLE views with fov_deg = 90 from `eye`, for square frames (w == h): the faces of a cube map in the order
    +x -x +y -y +z -z.  Image x runs along axis_x (to the viewer's right), image y upwards along axis_y:
        face   axis_z (forward)   axis_y (up)   axis_x (right = forward x up)
        +x     ( 1, 0, 0)         (0, 1, 0)     ( 0, 0, 1)
        -x     (-1, 0, 0)         (0, 1, 0)     ( 0, 0,-1)
        +y     ( 0, 1, 0)         (0, 0, 1)     ( 1, 0, 0)
        -y     ( 0,-1, 0)         (0, 0,-1)     ( 1, 0, 0)
        +z     ( 0, 0, 1)         (0, 1, 0)     (-1, 0, 0)
        -z     ( 0, 0,-1)         (0, 1, 0)     ( 1, 0, 0)"""
    faces = [((0, 0, 1), (0, 1, 0), (1, 0, 0)), ((0, 0, -1), (0, 1, 0), (-1, 0, 0)), ((1, 0, 0), (0, 0, 1), (0, 1, 0)),
             ((1, 0, 0), (0, 0, -1), (0, -1, 0)), ((-1, 0, 0), (0, 1, 0), (0, 0, 1)), ((1, 0, 0), (0, 1, 0), (0, 0, -1))]
    return [view(RT_VIEW_PINHOLE, eye, ax, ay, az, fov_deg=90) for ax, ay, az in faces]


def stereo_views(v, separation):
    """-> (left, right): two copies of the view whose origins are moved by -/+ separation / 2 along the unit axis_x:
    origin[c] -/+ u[c] * (separation / 2.0) with u = normal3d(axis_x).  (With lookAt's basis, whose axis_x points left, the first is
    the viewer's right eye.)"""
    u = normal3d(list(v.axis_x))
    half = float(separation) / 2.0
    left, right = _copy_view(v), _copy_view(v)
    for c in range(3):
        left.origin[c] = v.origin[c] - float(u[c]) * half
        right.origin[c] = v.origin[c] + float(u[c]) * half
    return left, right


def equirect_tables(w, h, lib=None):
    """-> (lon, lat): the panorama's tables for a w x h view (rt_view_equirect_tables): float64 arrays of 2 w and 2 h entries on 16-byte
    boundaries, {sin, cos} of the longitude 2 pi (x + 0.5) / w - pi per column and of the latitude pi / 2 - pi (y + 0.5) / h per row."""
    lib = lib or load_library()
    lon, lat = _aligned_f64(2 * w), _aligned_f64(2 * h)
    _check(lib, lib.rt_view_equirect_tables(w, h, C.c_void_p(lon.ctypes.data), C.c_void_p(lat.ctypes.data)), "rt_view_equirect_tables")
    return lon, lat


def view_work_bytes(w, h, lib=None):
    """Bytes of device workspace Renderer.trace_view prefers for a w x h view (host arithmetic; 0 for a size it refuses).  48 w - one
    row - is the least it accepts."""
    return int((lib or load_library()).rt_view_work_bytes(w, h))


def view_rays(v, w, h, first_row=0, rows=None, lib=None):
    """The host probe (rt_view_rays): rows [first_row, first_row + rows) (default: to the last) of the view's w x h primary rays as an
    (rows * w, 6) float64 array {org, dir} in row order - what the GPU generates, bit for bit.  No GPU."""
    import numpy as np
    lib = lib or load_library()
    rows = h - first_row if rows is None else rows
    out = np.empty((max(rows, 0) * w, 6), np.float64)
    _check(lib, lib.rt_view_rays(C.byref(v), w, h, first_row, rows, C.c_void_p(out.ctypes.data)), "rt_view_rays")
    return out


def trace_view(scene, v, w, h, segs=0, want=("rgba",), lib=None):
    """trace_view(scene, view, w, h) -> the dict of trace_rays for the view's w x h rays in frame order (ray y w + x; "rgba" (w h, 4)
    uint8 is the frame), on GPU 0 with rt_render's resident scene.  The rays are generated on the GPU: none crosses the link (an
    EQUIRECT view's tables, host memory here, are uploaded once)."""
    import numpy as np
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    want = set(want)
    if not want or want - {"rgb", "rgba", "hits"}:
        raise ValueError("want names some of 'hits', 'rgb', 'rgba'")
    n = w * h
    out = {}
    if "rgb" in want:
        out["rgb"] = np.empty((n, 3), np.float64)
    if "rgba" in want:
        out["rgba"] = np.empty((n, 4), np.uint8)
    records = (RtHit * max(n, 1))() if "hits" in want else None
    bufs = RtRayOutputs(out["rgb"].ctypes.data if "rgb" in out else None, out["rgba"].ctypes.data if "rgba" in out else None,
                        C.addressof(records) if records is not None else None)
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    _check(lib, lib.rt_trace_view(buf, len(blob), C.byref(v), w, h, segs, C.byref(bufs), None), "rt_trace_view")
    if records is not None:
        out["hits"] = [_hit_dict(r) for r in records[:n]]
    return out


# --------------------------------------------------------------------------- sampled views: sub-pixel offsets and a thin lens
def _samples_array(samples):
    """-> (a ctypes array of RtViewSample or None, n), from a list of RtViewSample or of (dx, dy, lu, lv) tuples."""
    samples = list(samples) if samples is not None else []
    n = len(samples)
    if n == 0:
        return None, 0
    arr = (RtViewSample * n)()
    for i, s in enumerate(samples):
        arr[i] = s if isinstance(s, RtViewSample) else RtViewSample(*(float(c) for c in s))
    return arr, n


def view_sample(dx=0.0, dy=0.0, lu=0.0, lv=0.0):
    """-> RtViewSample: a sub-pixel offset in pixels (dy downwards) and a lens point on the unit disk."""
    return RtViewSample(float(dx), float(dy), float(lu), float(lv))


def lens(radius, focus):
    """-> RtViewLens: a thin lens of `radius` (along axis_x / axis_y) focused on the plane `focus` away along axis_z (PINHOLE views)."""
    return RtViewLens(float(radius), float(focus))


def view_samples_grid(k, lib=None):
    """-> the k x k grid pattern (rt_view_samples_grid), k in 1..32: a list of k k RtViewSample, sample j k + i with
    dx = (i + 0.5) / k - 0.5, dy = (j + 0.5) / k - 0.5 and (lu, lv) the concentric map of (2 dx, 2 dy) onto the unit disk."""
    lib = lib or load_library()
    arr = (RtViewSample * max(k * k, 1))()
    _check(lib, lib.rt_view_samples_grid(k, arr), "rt_view_samples_grid")
    return list(arr)


def equirect_sample_tables(w, h, samples, lib=None):
    """-> (lon, lat): the panorama's tables of len(samples) samples, one table per sample back to back (rt_view_equirect_sample_tables):
    float64 arrays of n 2 w and n 2 h entries on 16-byte boundaries."""
    lib = lib or load_library()
    arr, n = _samples_array(samples)
    lon, lat = _aligned_f64(2 * w * n), _aligned_f64(2 * h * n)
    _check(lib, lib.rt_view_equirect_sample_tables(w, h, n, arr, C.c_void_p(lon.ctypes.data), C.c_void_p(lat.ctypes.data)), "rt_view_equirect_sample_tables")
    return lon, lat


def view_samples_work_bytes(w, h, lib=None):
    """Bytes of device workspace Renderer.trace_view_samples prefers for a w x h view (host arithmetic; 0 for a size it refuses).
    96 w - one row - is the least it accepts."""
    return int((lib or load_library()).rt_view_samples_work_bytes(w, h))


def view_sample_rays(v, w, h, sample, lens=None, table=0, first_row=0, rows=None, lib=None):
    """The host probe for ONE sample (rt_view_sample_rays): rows [first_row, first_row + rows) of the sample's rays as an
    (rows * w, 6) float64 array - what the GPU generates, bit for bit.  `table`: which of an EQUIRECT view's tables to read.  No GPU."""
    import numpy as np
    lib = lib or load_library()
    rows = h - first_row if rows is None else rows
    out = np.empty((max(rows, 0) * w, 6), np.float64)
    s = sample if isinstance(sample, RtViewSample) else RtViewSample(*(float(c) for c in sample))
    _check(lib, lib.rt_view_sample_rays(C.byref(v), w, h, C.byref(lens) if lens is not None else None, C.byref(s), table, first_row, rows,
                                        C.c_void_p(out.ctypes.data)), "rt_view_sample_rays")
    return out


def trace_view_samples(scene, v, w, h, samples, lens=None, segs=0, want=("rgba",), lib=None):
    """trace_view_samples(scene, view, w, h, samples) -> {"rgb": (w h, 3) float64, "rgba": (w h, 4) uint8} (the keys named in `want`):
    the mean of len(samples) traces of the view, one per sample, averaged on GPU 0 with rt_render's resident scene
    (rt_trace_view_samples).  An EQUIRECT view's tables are equirect_sample_tables(w, h, samples)."""
    import numpy as np
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    want = set(want)
    if not want or want - {"rgb", "rgba"}:
        raise ValueError("want names some of 'rgb', 'rgba'")
    arr, n = _samples_array(samples)
    px = w * h
    out = {}
    if "rgb" in want:
        out["rgb"] = np.empty((px, 3), np.float64)
    if "rgba" in want:
        out["rgba"] = np.empty((px, 4), np.uint8)
    bufs = RtRayOutputs(out["rgb"].ctypes.data if "rgb" in out else None, out["rgba"].ctypes.data if "rgba" in out else None, None)
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    _check(lib, lib.rt_trace_view_samples(buf, len(blob), C.byref(v), w, h, C.byref(lens) if lens is not None else None, n, arr, segs, C.byref(bufs), None),
           "rt_trace_view_samples")
    return out


def _points3(a, what, n=None):
    import numpy as np
    a = np.asarray(a)
    if a.dtype.kind not in "fiu" or a.ndim != 2 or a.shape[1] != 3 or (n is not None and a.shape[0] != n):
        raise ValueError("%s must be an (n, 3) array of numbers" % what)
    return a.astype(np.float64)


def _skip_array(skip, n):
    import numpy as np
    a = np.asarray(skip)
    if a.dtype.kind not in "iu" or a.shape != (n,):
        raise ValueError("skip must be n integers (sphere indices in blob order; -1 = none)")
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError("skip must fit 32 bits")
    return np.ascontiguousarray(a, np.int32)


def light_segments(scene, points, facing=None, skip=None):
    """The segments of the reference's light loop (main.js:286-292) from `points` ((n, 3): hit.p) to every light of the scene dict, in
    numpy with the reference's operation order: shadow_vec = light - point, light_mag = (x x + y y) + z z, light_len = sqrt(light_mag),
    shadow_vec * (1 / light_len) where light_len != 0, shadow_dot = (s0 l0 + s1 l1) + s2 l2 with l = `facing` ((n, 3): hit.l, the normal
    turned towards the ray's side).  Returns one dict per light: "rays" (n, 6) {point, shadow_vec} as occlusion takes them, "length"
    (light_len), "light_mag", "shadow_dot" and "mask" (shadow_dot > 0: the surface faces the light) - without `facing` shadow_dot is
    None and the mask all True - and "skip" (the int32 copy of `skip`, hit_i per point, or None)."""
    import numpy as np
    p = _points3(points, "points")
    n = p.shape[0]
    l = _points3(facing, "facing", n) if facing is not None else None
    sk = _skip_array(skip, n) if skip is not None else None
    out = []
    for light in np.array(light_positions(scene["lights"]), np.float64).reshape(-1, 3):
        v = light[None, :] - p
        mag = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        length = np.sqrt(mag)
        with np.errstate(divide="ignore"):
            k = np.where(length != 0.0, 1.0 / length, 1.0)
        v = np.where((length != 0.0)[:, None], v * k[:, None], v)
        rays = np.empty((n, 6), np.float64)
        rays[:, 0:3] = p
        rays[:, 3:6] = v
        dot = (v[:, 0] * l[:, 0] + v[:, 1] * l[:, 1]) + v[:, 2] * l[:, 2] if l is not None else None
        out.append({"rays": rays, "length": length, "light_mag": mag, "shadow_dot": dot,
                    "mask": dot > 0.0 if dot is not None else np.ones(n, bool), "skip": sk})
    return out


def occlusion(scene, rays, length=None, intensity=None, skip=None, want=("intensity",), lib=None, order="list"):
    """occlusion(scene, rays) -> {"intensity": (n,) float64, "blocker": (n,) int32} (the keys named in `want`): the reference's shadow
    scan (main.js:293-304) per row {org, dir} of the float64 (n, 6) array `rays`, directions as given, on GPU 0 with rt_render's
    resident scene.  Per ray: `length` (light_len; None = +Infinity), `intensity` (what the scan starts with; None = the scene's
    light_intensity), `skip` (hit_i, the sphere left out, blob order; None or a value outside the scene = none).  The scan goes through the
    spheres in blob order: a sphere met before `length` divides the intensity by its albedo[4], or - albedo[4] == 0 - makes it 0, becomes
    the blocker and ends the scan.  A ray with a non-finite component is not traced: NaN, -1.  order: "list", or "binned"
    (rt_occlusion_binned: the GPU orders each chunk of 2^18 rays first - the same results)."""
    import numpy as np
    if order not in ("list", "binned"):
        raise ValueError("order is 'list' or 'binned'")
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    want = set(want)
    if not want or want - {"intensity", "blocker"}:
        raise ValueError("want names some of 'intensity', 'blocker'")
    rays = np.asarray(rays)
    if rays.dtype.kind not in "fiu" or rays.ndim != 2 or rays.shape[1] != 6:
        raise ValueError("rays must be an (n, 6) array: org[3], dir[3] per row")
    n = rays.shape[0]
    if n == 0:
        raise ValueError("rays must not be empty")
    aligned = np.empty(n * 6 + 2, np.float64)             # a contiguous copy on a 16-byte boundary
    aligned = aligned[(aligned.ctypes.data >> 3) & 1:][:n * 6]
    aligned[:] = rays.reshape(-1)
    per_ray = {}
    for name, a in (("length", length), ("intensity", intensity)):
        if a is not None:
            a = np.asarray(a)
            if a.dtype.kind not in "fiu" or a.shape != (n,):
                raise ValueError("%s must be n numbers" % name)
            per_ray[name] = np.ascontiguousarray(a, np.float64)
    if skip is not None:
        per_ray["skip"] = _skip_array(skip, n)
    out = {}
    if "intensity" in want:
        out["intensity"] = np.empty(n, np.float64)
    if "blocker" in want:
        out["blocker"] = np.empty(n, np.int32)
    ins = RtOcclusionInputs(*[per_ray[k].ctypes.data if k in per_ray else None for k in ("length", "intensity", "skip")])
    bufs = RtOcclusionOutputs(*[out[k].ctypes.data if k in out else None for k in ("intensity", "blocker")])
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    call, what = (lib.rt_occlusion, "rt_occlusion") if order == "list" else (lib.rt_occlusion_binned, "rt_occlusion_binned")
    _check(lib, call(buf, len(blob), n, C.c_void_p(aligned.ctypes.data), C.byref(ins), C.byref(bufs), None), what)
    return out


def light_intensity_at(scene, points, facing, skip, lib=None, order="list"):
    """The light intensity the reference's whole light loop (main.js:283-305) leaves at `points` ((n, 3) hit.p, with `facing` hit.l and
    `skip` hit_i per point) of the scene dict: the lights in order, ONE intensity carried from light to light (quirk q2: glass a first
    light's segment crossed has raised it for the second, and a blocked first light has zeroed it), a light the surface does not face
    (shadow_dot <= 0) leaves it as it is.  One occlusion call per light over the points that face it.  -> (n,) float64."""
    import numpy as np
    segs = light_segments(scene, points, facing, skip)
    n = np.asarray(points).shape[0]
    li = np.full(n, float(scene.get("light_intensity", 50)), np.float64)
    for sg in segs:
        m = sg["mask"]
        if not m.any():
            continue
        got = occlusion(scene, sg["rays"][m], length=sg["length"][m], intensity=li[m], skip=sg["skip"][m] if sg["skip"] is not None else None,
                        want=("intensity",), lib=lib, order=order)
        li[m] = got["intensity"]
    return li


# --------------------------------------------------------------------------- ambient occlusion (include/rt_hip.h: rt_ambient)
def hit_records(points, normals, objects, inside=None):
    """-> an (n,) HIT_DTYPE array: receivers for ambient() made by hand - `points` and `normals` (n, 3), `objects` n sphere indices in
    blob order (the sphere the point lies on, left out of its scans; -1: a miss, not scanned), `inside` n flags (the normal is turned
    round; None = all outside).  t, u and v are 0: ambient occlusion does not read them."""
    import numpy as np
    p = _points3(points, "points")
    n = p.shape[0]
    out = np.zeros(n, np.dtype(HIT_FIELDS))
    out["point"] = p
    out["normal"] = _points3(normals, "normals", n)
    out["object"] = _skip_array(objects, n)
    if inside is not None:
        ins = np.asarray(inside)
        if ins.shape != (n,):
            raise ValueError("inside must be n flags")
        out["inside"] = ins.astype(bool)
    return out


def _hits_array(hits):
    """-> a contiguous HIT_DTYPE array from one, or from a list of hit dicts as trace_rays / trace_view return them (None: a miss)."""
    import numpy as np
    dt = np.dtype(HIT_FIELDS)
    if isinstance(hits, np.ndarray):
        if hits.dtype != dt or hits.ndim != 1:
            raise ValueError("hits must be an (n,) array of HIT_DTYPE")
        return np.ascontiguousarray(hits)
    out = np.zeros(len(hits), dt)
    for i, r in enumerate(hits):
        if r is None:
            out[i]["object"], out[i]["t"] = -1, float("inf")
        else:
            out[i] = (r["object"], int(r["inside"]), r["t"], r["point"], r["normal"], r["u"], r["v"])
    return out


def view_hit_records(scene, v, w, h, lib=None):
    """-> the (w h,) HIT_DTYPE array of trace_view's "hits" output as the library wrote it: the receivers of ambient_view."""
    import numpy as np
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    out = np.zeros(w * h, np.dtype(HIT_FIELDS))
    bufs = RtRayOutputs(None, None, out.ctypes.data)
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    _check(lib, lib.rt_trace_view(buf, len(blob), C.byref(v), w, h, 0, C.byref(bufs), None), "rt_trace_view")
    return out


def ambient_dirs(n, lib=None):
    """-> (n, 3) float64: the cosine-weighted spiral of rt_ambient_cosine_dirs, local directions with z along the facing normal: entry k
    is {r cos(phi), r sin(phi), sqrt(1 - u)} with u = (k + 0.5) / n, phi = k pi (3 - sqrt(5)), r = sqrt(u) (fdlibm's cos and sin: the same
    bits on every host)."""
    import numpy as np
    lib = lib or load_library()
    out = np.empty((max(n, 0), 3), np.float64)
    _check(lib, lib.rt_ambient_cosine_dirs(n, C.c_void_p(out.ctypes.data)), "rt_ambient_cosine_dirs")
    return out


def _ambient_args(n_samples, radius, dirs, stride, base, lib):
    import numpy as np
    if dirs is None:
        dirs = ambient_dirs(n_samples, lib)
    dirs = np.ascontiguousarray(dirs, np.float64)
    if dirs.ndim != 2 or dirs.shape[1] != 3:
        raise ValueError("dirs must be an (n_dirs, 3) array: local directions, z along the facing normal")
    return RtAmbient(n_samples, dirs.shape[0], stride, 0, base, float(radius)), dirs


def ambient_segments(hits, sample, n_samples, dirs=None, stride=1, base=0, lib=None):
    """The host probe (rt_ambient_segments): -> (rays (n, 6) float64, skip (n,) int32), the segments sample `sample` of the receivers
    `hits` scans - what the GPU generates, bit for bit.  dirs: None = ambient_dirs(n_samples).  No GPU."""
    import numpy as np
    lib = lib or load_library()
    h = _hits_array(hits)
    a, dirs = _ambient_args(n_samples, 1.0, dirs, stride, base, lib)
    rays, skip = np.empty((len(h), 6), np.float64), np.empty(len(h), np.int32)
    _check(lib, lib.rt_ambient_segments(C.byref(a), C.c_void_p(dirs.ctypes.data), len(h), C.c_void_p(h.ctypes.data), sample, C.c_void_p(rays.ctypes.data),
                                        C.c_void_p(skip.ctypes.data)), "rt_ambient_segments")
    return rays, skip


def _ambient_outputs(n, want):
    import numpy as np
    want = set(want)
    if not want or want - {"open", "intensity", "rgba"}:
        raise ValueError("want names some of 'open', 'intensity', 'rgba'")
    out = {}
    if "open" in want:
        out["open"] = np.empty(n, np.float64)
    if "intensity" in want:
        out["intensity"] = np.empty(n, np.float64)
    if "rgba" in want:
        out["rgba"] = np.empty((n, 4), np.uint8)
    return out, RtAmbientOutputs(*[out[k].ctypes.data if k in out else None for k in ("open", "intensity", "rgba")])


def ambient(scene, hits, n_samples, radius, dirs=None, stride=1, want=("open",), order="list", base=0, lib=None):
    """ambient(scene, hits, n_samples, radius) -> {"open": (n,) float64, "intensity": (n,) float64, "rgba": (n, 4) uint8} (the keys named
    in `want`): ambient occlusion of the receivers `hits` (a HIT_DTYPE array - view_hit_records, hit_records - or a list of hit dicts) on
    GPU 0 with rt_render's resident scene.  Per receiver n_samples shadow scans of length `radius` (float("inf"): sky visibility) leave the
    point along directions of the hemisphere around its facing normal, the receiver's own sphere left out: open is the share of scans
    no opaque sphere ended (a miss: 1.0), intensity their mean intensity starting from 1.0 (glass DIVIDES by albedo[4], quirk q2: it can
    exceed 1; NaN for a miss), rgba open as a grey pixel.  dirs: (n_dirs, 3) local directions, None = ambient_dirs(n_samples); sample s of
    receiver i uses entry ((base + i) stride + s) % n_dirs - stride 0: the same directions everywhere.  order: "list" (the only one:
    receivers that come from a view are neighbours already)."""
    if order != "list":
        raise ValueError("order is 'list'")
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    h = _hits_array(hits)
    if len(h) == 0:
        raise ValueError("hits must not be empty")
    a, dirs = _ambient_args(n_samples, radius, dirs, stride, base, lib)
    out, bufs = _ambient_outputs(len(h), want)
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    _check(lib, lib.rt_ambient(buf, len(blob), C.byref(a), C.c_void_p(dirs.ctypes.data), len(h), C.c_void_p(h.ctypes.data), C.byref(bufs), None), "rt_ambient")
    return out


def ambient_view_work_bytes(w, h, lib=None):
    """Bytes of device workspace Renderer.ambient_view prefers for a w x h view (host arithmetic; 0 for a size it refuses).  128 w - one
    row - is the least it accepts."""
    return int((lib or load_library()).rt_ambient_view_work_bytes(w, h))


def ambient_view(scene, v, w, h, n_samples, radius, dirs=None, stride=1, want=("rgba",), base=0, lib=None):
    """ambient() of what the view sees at w x h, in frame order ("rgba" (w h, 4) uint8 is the grey frame): the view's rays, their hit
    records and the scans are made on the GPU (rt_ambient_view) - only the direction table goes up and the results come back."""
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    a, dirs = _ambient_args(n_samples, radius, dirs, stride, base, lib)
    out, bufs = _ambient_outputs(w * h, want)
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    _check(lib, lib.rt_ambient_view(buf, len(blob), C.byref(v), w, h, C.byref(a), C.c_void_p(dirs.ctypes.data), C.byref(bufs), None), "rt_ambient_view")
    return out


# --------------------------------------------------------------------------- gathered light (include/rt_hip.h: rt_gather)
def _gather_args(n, n_samples, dirs, stride, segs, base, pix_base, pix_stride, lib):
    import numpy as np
    if dirs is None:
        dirs = ambient_dirs(n_samples, lib)
    dirs = np.ascontiguousarray(dirs, np.float64)
    if dirs.ndim != 2 or dirs.shape[1] != 3:
        raise ValueError("dirs must be an (n_dirs, 3) array: local directions, z along the facing normal")
    return RtGather(n_samples, dirs.shape[0], stride, segs, base, pix_base, n if pix_stride is None else pix_stride), dirs


def _gather_outputs(n, want):
    import numpy as np
    want = set(want)
    if not want or want - {"rgb", "rgba"}:
        raise ValueError("want names some of 'rgb', 'rgba'")
    out = {}
    if "rgb" in want:
        out["rgb"] = np.empty((n, 3), np.float64)
    if "rgba" in want:
        out["rgba"] = np.empty((n, 4), np.uint8)
    return out, RtGatherOutputs(*[out[k].ctypes.data if k in out else None for k in ("rgb", "rgba")])


def gather(scene, hits, n_samples, dirs=None, stride=1, segs=0, base=0, pix_base=0, pix_stride=None, want=("rgb",), lib=None, mapping="receivers",
           weights=None):
    """gather(scene, hits, n_samples) -> {"rgb": (n, 3) float64, "rgba": (n, 4) uint8} (the keys named in `want`): the light that arrives
    at the receivers `hits` (a HIT_DTYPE array - view_hit_records, hit_records - or a list of hit dicts) from the rest of the scene, on
    GPU 0 with rt_render's resident scene.  Per receiver n_samples rays leave the point along the directions ambient_segments defines
    (dirs: (n_dirs, 3) local directions, None = ambient_dirs(n_samples), with which rgb is irradiance / pi; sample s of receiver i uses
    entry ((base + i) stride + s) % n_dirs), each traced as trace_rays traces any ray - depth `segs` (0: the scene's), no sphere left out
    - and rgb is their mean, rgba that mean as a pixel.  A miss or a NaN record gives NaN x 3 and 0, 0, 0, 255.  The stars sampler's pix of
    sample s of receiver i is pix_base + s pix_stride + i; pix_stride None = len(hits).
    mapping: "receivers" (one lane per receiver: rt_gather, for lists of thousands) or "samples" (one workgroup per receiver, its samples
    on lanes: rt_gather_probes, for short lists - the same bytes; docs/EVIDENCE.md, "Probes", has the crossover).  weights: an
    (n_dirs, n_weights) float64 table, n_weights 1..16, with mapping "samples" only; `want` may then name "coef": (n, n_weights, 3)
    float64, the mean over the samples of weights[e_s][k] c_s (e_s: the entry sample s took its direction from)."""
    if mapping not in ("receivers", "samples"):
        raise ValueError("mapping is 'receivers' or 'samples'")
    if weights is not None and mapping != "samples":
        raise ValueError("weights need mapping='samples'")
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    h = _hits_array(hits)
    if len(h) == 0:
        raise ValueError("hits must not be empty")
    a, dirs = _gather_args(len(h), n_samples, dirs, stride, segs, base, pix_base, pix_stride, lib)
    if mapping == "receivers":
        out, bufs = _gather_outputs(len(h), want)
        _init_once(lib)
        buf = C.create_string_buffer(blob, len(blob))
        _check(lib, lib.rt_gather(buf, len(blob), C.byref(a), C.c_void_p(dirs.ctypes.data), len(h), C.c_void_p(h.ctypes.data), C.byref(bufs), None), "rt_gather")
        return out
    import numpy as np
    n_weights = 0
    if weights is not None:
        weights = np.ascontiguousarray(weights, np.float64)
        if weights.ndim != 2 or weights.shape[0] != dirs.shape[0]:
            raise ValueError("weights must be an (n_dirs, n_weights) array: one row per table entry")
        n_weights = weights.shape[1]
    want = set(want)
    if "coef" in want and weights is None:
        raise ValueError("'coef' needs weights")
    if weights is not None and "coef" not in want:
        raise ValueError("weights are given: want names 'coef'")
    out, plain = _gather_outputs(len(h), want - {"coef"}) if want - {"coef"} else ({}, RtGatherOutputs(None, None))
    if "coef" in want:
        out["coef"] = np.empty((len(h), n_weights, 3), np.float64)
    bufs = RtProbeOutputs(plain.rgb, plain.rgba, out["coef"].ctypes.data if "coef" in out else None)
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    _check(lib, lib.rt_gather_probes(buf, len(blob), C.byref(a), C.c_void_p(dirs.ctypes.data), C.c_void_p(weights.ctypes.data if weights is not None else 0),
                                     n_weights, len(h), C.c_void_p(h.ctypes.data), C.byref(bufs), None), "rt_gather_probes")
    return out


def sh9_weights(dirs, lib=None):
    """-> (n, 9) float64: rt_probe_sh9_weights, the nine real spherical harmonics of bands 0..2 at the directions `dirs` (n, 3), taken as
    given, in the header's order: 1, y, z, x, xy, yz, xz, 3 z z - 1, x x - y y, each with its constant.  A weight table for gather().
    No GPU."""
    import numpy as np
    lib = lib or load_library()
    dirs = np.ascontiguousarray(dirs, np.float64)
    if dirs.ndim != 2 or dirs.shape[1] != 3:
        raise ValueError("dirs must be an (n, 3) array")
    out = np.empty((dirs.shape[0], 9), np.float64)
    _check(lib, lib.rt_probe_sh9_weights(dirs.shape[0], C.c_void_p(dirs.ctypes.data), C.c_void_p(out.ctypes.data)), "rt_probe_sh9_weights")
    return out


def probe_records(points):
    """-> the hit records probes() gathers at: `points` (n, 3) in free space as receivers with normal (0, 0, 1) on object 0.  The frame
    of that normal is the world's axes, so a table's directions are world directions."""
    import numpy as np
    p = _points3(points, "points")
    normals = np.zeros_like(p)
    normals[:, 2] = 1.0
    return hit_records(p, normals, np.zeros(len(p), np.int32))


def probes(scene, points, n_samples, dirs=None, weights=None, segs=0, pix_base=0, want=("rgb",), lib=None):
    """Light probes at `points` (n, 3) in free space: gather(mapping="samples", stride=0) of probe_records(points) - every probe takes
    the table's first n_samples directions, as world directions.  dirs: None = lighting_offsets(n_samples), the spiral over the whole
    sphere.  weights as gather takes them: sh9_weights(dirs) with want=("coef",) gives each probe's nine spherical-harmonics
    coefficients per channel, up to the factor 4 pi."""
    lib = lib or load_library()
    if dirs is None:
        dirs = lighting_offsets(n_samples, lib)
    return gather(scene, probe_records(points), n_samples, dirs=dirs, stride=0, segs=segs, pix_base=pix_base, want=want, lib=lib, mapping="samples",
                  weights=weights)


def gather_view_work_bytes(w, h, lib=None):
    """Bytes of device workspace Renderer.gather_view prefers for a w x h view (host arithmetic; 0 for a size it refuses).  128 w - one
    row - is the least it accepts."""
    return int((lib or load_library()).rt_gather_view_work_bytes(w, h))


def gather_view(scene, v, w, h, n_samples, dirs=None, stride=1, segs=0, base=0, pix_base=0, pix_stride=None, want=("rgba",), lib=None):
    """gather() of what the view sees at w x h, in frame order ("rgba" (w h, 4) uint8 is the frame): the view's rays, their hit records
    and the gathered rays are made on the GPU (rt_gather_view) - only the direction table goes up and the results come back.
    pix_stride None = w h, the sampled view's pix = s w h + y w + x."""
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    a, dirs = _gather_args(w * h, n_samples, dirs, stride, segs, base, pix_base, pix_stride, lib)
    out, bufs = _gather_outputs(w * h, want)
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    _check(lib, lib.rt_gather_view(buf, len(blob), C.byref(v), w, h, C.byref(a), C.c_void_p(dirs.ctypes.data), C.byref(bufs), None), "rt_gather_view")
    return out


# --------------------------------------------------------------------------- sampled lights (include/rt_hip.h: rt_lighting)
LIGHTING_OUTPUTS = ("diffuse", "intensity", "lit", "rgba")


def lighting_offsets(n, lib=None):
    """-> (n, 3) float64: rt_lighting_sphere_offsets' spiral of n points on the unit sphere: entry k is {r cos(phi), r sin(phi), z} with
    z = 1 - (2 k + 1) / n, r = sqrt(1 - z z), phi = k pi (3 - sqrt(5)) (fdlibm's cos and sin: the same bits on every host).  Consecutive
    entries lie on a ring: use whole sets (stride = n_samples over a table of sets), not neighbours of one long spiral."""
    import numpy as np
    lib = lib or load_library()
    out = np.empty((max(n, 0), 3), np.float64)
    _check(lib, lib.rt_lighting_sphere_offsets(n, C.c_void_p(out.ctypes.data)), "rt_lighting_sphere_offsets")
    return out


def _lighting_args(n_samples, light_radius, offs, stride, base, lib):
    import numpy as np
    if offs is None:
        offs = lighting_offsets(n_samples, lib)
    offs = np.ascontiguousarray(offs, np.float64)
    if offs.ndim != 2 or offs.shape[1] != 3:
        raise ValueError("offs must be an (n_offs, 3) array: offsets of a light, in units of light_radius")
    return RtLighting(n_samples, offs.shape[0], stride, 0, base, float(light_radius)), offs


def lighting_segments(scene_or_lights, hits, sample, light, n_samples, light_radius, offs=None, stride=1, base=0, lib=None):
    """The host probe (rt_lighting_segments): the segments of (`sample`, `light`) of the receivers `hits` towards light `light` of a
    scene dict (or of an (n_lights, 3) array of positions), displaced by light_radius times the sample's table entry - what the GPU
    builds in registers, bit for bit.  -> a dict in light_segments' layout: "rays" (n, 6) {point, shadow_vec}, "length" (light_len),
    "light_mag", "shadow_dot" (against hit.l, the normal on the ray's side), "mask" (not shadow_dot <= 0, and scanned: the loop goes on
    to the scan) and "skip" (n,) int32 (hit_i; -1 for a receiver that is not scanned, whose other entries are NaN).  offs: None =
    lighting_offsets(n_samples).  No GPU."""
    import numpy as np
    lib = lib or load_library()
    h = _hits_array(hits)
    xyz = np.array(light_positions(scene_or_lights["lights"] if isinstance(scene_or_lights, dict) else scene_or_lights), np.float64).reshape(-1, 3)
    a, offs = _lighting_args(n_samples, light_radius, offs, stride, base, lib)
    n = len(h)
    rays, skip = np.empty((n, 6), np.float64), np.empty(n, np.int32)
    length, mag, dot = np.empty(n, np.float64), np.empty(n, np.float64), np.empty(n, np.float64)
    _check(lib, lib.rt_lighting_segments(C.byref(a), C.c_void_p(offs.ctypes.data), len(xyz), C.c_void_p(xyz.ctypes.data), n, C.c_void_p(h.ctypes.data), sample,
                                         light, C.c_void_p(rays.ctypes.data), C.c_void_p(length.ctypes.data), C.c_void_p(mag.ctypes.data),
                                         C.c_void_p(dot.ctypes.data), C.c_void_p(skip.ctypes.data)), "rt_lighting_segments")
    with np.errstate(invalid="ignore"):
        mask = ~(dot <= 0.0) & (skip >= 0)
    return {"rays": rays, "length": length, "light_mag": mag, "shadow_dot": dot, "mask": mask, "skip": skip}


def _lighting_outputs(n, want):
    import numpy as np
    want = set(want)
    if not want or want - set(LIGHTING_OUTPUTS):
        raise ValueError("want names some of 'diffuse', 'intensity', 'lit', 'rgba'")
    out = {k: (np.empty((n, 4), np.uint8) if k == "rgba" else np.empty(n, np.float64)) for k in LIGHTING_OUTPUTS if k in want}
    return out, RtLightingOutputs(*[out[k].ctypes.data if k in out else None for k in LIGHTING_OUTPUTS])


def lighting(scene, hits, n_samples=1, light_radius=0.0, offs=None, stride=1, want=("diffuse",), base=0, lib=None):
    """lighting(scene, hits) -> {"diffuse", "intensity", "lit": (n,) float64, "rgba": (n, 4) uint8} (the keys named in `want`): how much
    light arrives at the receivers `hits` (a HIT_DTYPE array - view_hit_records, hit_records - or a list of hit dicts), by the
    reference's light loop (main.js:283-306) on GPU 0 with rt_render's resident scene.  With the defaults it is the reference's own loop:
    intensity is light_intensity_at's number, min(1, diffuse) * albedo[1] the reference's diffuse_intensity.  With n_samples > 1 and a
    light_radius the loop runs n_samples times, every light displaced by light_radius times an entry of `offs` ((n_offs, 3); None =
    lighting_offsets(n_samples); sample s of receiver i uses entry ((base + i) stride + s) % n_offs for every light), and the results are
    averaged: soft shadows.  diffuse is the raw sum (li * shadow_dot / light_mag over the lights that arrive), lit the share of (sample,
    light) pairs that arrived, rgba min(1, diffuse) as a grey pixel.  A receiver that is not scanned (a miss, a non-finite record): NaN,
    NaN, 0.0, opaque black."""
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    h = _hits_array(hits)
    if len(h) == 0:
        raise ValueError("hits must not be empty")
    a, offs = _lighting_args(n_samples, light_radius, offs, stride, base, lib)
    out, bufs = _lighting_outputs(len(h), want)
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    _check(lib, lib.rt_lighting(buf, len(blob), C.byref(a), C.c_void_p(offs.ctypes.data), len(h), C.c_void_p(h.ctypes.data), C.byref(bufs), None), "rt_lighting")
    return out


def lighting_view_work_bytes(w, h, lib=None):
    """Bytes of device workspace Renderer.lighting_view prefers for a w x h view (host arithmetic; 0 for a size it refuses).  128 w - one
    row - is the least it accepts."""
    return int((lib or load_library()).rt_lighting_view_work_bytes(w, h))


def lighting_view(scene, v, w, h, n_samples=1, light_radius=0.0, offs=None, stride=1, want=("rgba",), base=0, lib=None):
    """lighting() of what the view sees at w x h, in frame order ("rgba" (w h, 4) uint8 is the grey frame): the view's rays, their hit
    records and the light loops are made on the GPU (rt_lighting_view) - only the offset table goes up and the results come back."""
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    a, offs = _lighting_args(n_samples, light_radius, offs, stride, base, lib)
    out, bufs = _lighting_outputs(w * h, want)
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    _check(lib, lib.rt_lighting_view(buf, len(blob), C.byref(v), w, h, C.byref(a), C.c_void_p(offs.ctypes.data), C.byref(bufs), None), "rt_lighting_view")
    return out


# --------------------------------------------------------------------------- wavefront ray lists (include/rt_hip.h: rt_node)
def _node_dtype():
    import numpy as np
    return np.dtype(NODE_FIELDS)


def __getattr__(name):                                   # NODE_DTYPE, HIT_DTYPE: built on first use, so that importing this module does not need numpy
    if name == "NODE_DTYPE":
        return _node_dtype()
    if name == "HIT_DTYPE":
        import numpy as np
        return np.dtype(HIT_FIELDS)
    raise AttributeError(name)


def nodes_spawn_work_bytes(n, lib=None):
    """Bytes of device workspace Renderer.spawn_rays needs for n nodes (host arithmetic; 0 for n == 0 and n >= 2^31)."""
    return int((lib or load_library()).rt_nodes_spawn_work_bytes(n))


def shade_rays(scene, rays, pix=None, path=None, order="list", lib=None):
    """shade_rays(scene, rays) -> structured array (NODE_DTYPE), node i for row i {org, dir} of the float64 (n, 6) array `rays`: one level
    of intersectWorld (main.js:216-336 without its two recursive calls), directions as given, on GPU 0 with rt_render's resident scene.
    pix / path: n uint32 each, the stars sampler's pix and path per ray (None: i and 1).  order: "list", or "binned" (the GPU orders each
    chunk of 2^18 rays first - the same nodes)."""
    import numpy as np
    if order not in ("list", "binned"):
        raise ValueError("order is 'list' or 'binned'")
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    rays = np.asarray(rays)
    if rays.dtype.kind not in "fiu" or rays.ndim != 2 or rays.shape[1] != 6 or rays.shape[0] == 0:
        raise ValueError("rays must be a non-empty (n, 6) array: org[3], dir[3] per row")
    n = rays.shape[0]
    aligned = np.empty(n * 6 + 2, np.float64)             # a contiguous copy on a 16-byte boundary
    aligned = aligned[(aligned.ctypes.data >> 3) & 1:][:n * 6]
    aligned[:] = rays.reshape(-1)
    extra = {}
    for name, a in (("pix", pix), ("path", path)):
        if a is not None:
            a = np.asarray(a)
            if a.dtype.kind not in "iu" or a.shape != (n,) or (a.size and (int(a.min()) < 0 or int(a.max()) >= 2 ** 32)):
                raise ValueError("%s must be n integers in [0, 2^32)" % name)
            extra[name] = np.ascontiguousarray(a.astype(np.uint32))
    nodes = np.zeros(n, _node_dtype())
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    rc = lib.rt_shade_rays(buf, len(blob), n, C.c_void_p(aligned.ctypes.data), C.c_void_p(extra["pix"].ctypes.data if "pix" in extra else 0),
                           C.c_void_p(extra["path"].ctypes.data if "path" in extra else 0), 1 if order == "binned" else 0, C.c_void_p(nodes.ctypes.data), None)
    _check(lib, rc, "rt_shade_rays")
    return nodes


def _ray_list(rays):
    """-> (n, the rays as n * 6 contiguous float64 on a 16-byte boundary)"""
    import numpy as np
    rays = np.asarray(rays)
    if rays.dtype.kind not in "fiu" or rays.ndim != 2 or rays.shape[1] != 6 or rays.shape[0] == 0:
        raise ValueError("rays must be a non-empty (n, 6) array: org[3], dir[3] per row")
    aligned = _aligned_f64(rays.shape[0] * 6)
    aligned[:] = rays.reshape(-1)
    return rays.shape[0], aligned


def relight_rays(scene, rays, n_samples, light_radius, offs=None, stride=1, pix=None, path=None, order="list", base=0, lib=None):
    """relight_rays(scene, rays, n_samples, light_radius) -> structured array (NODE_DTYPE): shade_rays' nodes with soft lights - diffuse
    and specular are the means over n_samples runs of the light loop, every light displaced by light_radius times an entry of `offs`
    ((n_offs, 3); None = lighting_offsets(n_samples)) and each run's terms clamped and weighted as the reference does (main.js:316-317);
    every other byte of a node is shade_rays'.  Sample s of ray i uses entry ((base + pix_i) stride + s) % n_offs for every light, pix_i =
    pix[i], or i: a list cut in pieces gives the whole list's nodes when each piece passes its rays' indices as pix (they are the stars
    sampler's pix too).  path and order as shade_rays takes them."""
    import numpy as np
    if order not in ("list", "binned"):
        raise ValueError("order is 'list' or 'binned'")
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    n, aligned = _ray_list(rays)
    a, offs = _lighting_args(n_samples, light_radius, offs, stride, base, lib)
    extra = {}
    for name, v in (("pix", pix), ("path", path)):
        if v is not None:
            v = np.asarray(v)
            if v.dtype.kind not in "iu" or v.shape != (n,) or (v.size and (int(v.min()) < 0 or int(v.max()) >= 2 ** 32)):
                raise ValueError("%s must be n integers in [0, 2^32)" % name)
            extra[name] = np.ascontiguousarray(v.astype(np.uint32))
    nodes = np.zeros(n, _node_dtype())
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    rc = lib.rt_relight_rays(buf, len(blob), C.byref(a), C.c_void_p(offs.ctypes.data), n, C.c_void_p(aligned.ctypes.data),
                             C.c_void_p(extra["pix"].ctypes.data if "pix" in extra else 0), C.c_void_p(extra["path"].ctypes.data if "path" in extra else 0),
                             1 if order == "binned" else 0, C.c_void_p(nodes.ctypes.data), None)
    _check(lib, rc, "rt_relight_rays")
    return nodes


def soft_view_work_bytes(w, h, lib=None):
    """Bytes of device workspace Renderer.trace_view_soft prefers for a w x h view (host arithmetic; 0 for a size it refuses).  48 w - one
    row - is the least it accepts."""
    return int((lib or load_library()).rt_soft_view_work_bytes(w, h))


def _soft_outputs(n, want, counts_allowed):
    import numpy as np
    want = set(want)
    allowed = {"rgb", "rgba"} | ({"level_counts"} if counts_allowed else set())
    if not (want - {"level_counts"}) or want - allowed:
        raise ValueError("want names some of %s" % ", ".join(repr(k) for k in sorted(allowed)))
    out = {}
    if "rgb" in want:
        out["rgb"] = np.empty((n, 3), np.float64)
    if "rgba" in want:
        out["rgba"] = np.empty((n, 4), np.uint8)
    return want, out, RtRayOutputs(out["rgb"].ctypes.data if "rgb" in out else None, out["rgba"].ctypes.data if "rgba" in out else None, None)


def trace_rays_soft(scene, rays, n_samples, light_radius, offs=None, stride=1, levels=1, segs=0, order_levels=False, want=("rgba",), base=0, lib=None,
                    method="wavefront", order="list"):
    """trace_rays_soft(scene, rays, n_samples, light_radius) -> {"rgb": (n, 3) float64, "rgba": (n, 4) uint8, "level_counts": uint64[16]}
    (the keys named in `want`): trace_rays(method="wavefront") with the nodes of the first `levels` levels relit as relight_rays relights
    them - the reference's picture, colours, highlights, reflections and glass, with lights that have a size.  levels 1 softens what the
    rays themselves hit, levels >= the depth every bounce; levels 0 is the wavefront trace itself.  pix_i is the index of the ROOT ray
    at every level.  offs None = lighting_offsets(n_samples) with stride 0 (every ray the same n_samples entries).
    method: "wavefront" (the default: the level-by-level loop, rt_trace_rays_soft) or "recursive" (rt_trace_rays_soft_recursive: one
    launch per chunk of 2^18 rays, a per-lane stack instead of nodes in device memory - the same bytes; no "level_counts", no
    order_levels).  order, for the recursive method: "list", or "binned" (the GPU orders each chunk first - the same bytes)."""
    import numpy as np
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    if method not in ("wavefront", "recursive"):
        raise ValueError("method is 'wavefront' or 'recursive'")
    if order not in ("list", "binned"):
        raise ValueError("order is 'list' or 'binned'")
    if method == "wavefront" and order != "list":
        raise ValueError("order is the recursive method's (the wavefront method has order_levels)")
    if method == "recursive" and order_levels:
        raise ValueError("order_levels is the wavefront method's (the recursive method has order)")
    if levels < 0 or levels >= 2 ** 32:
        raise ValueError("levels is a count of levels, 0 .. 2^32 - 1")
    n, aligned = _ray_list(rays)
    want, out, bufs = _soft_outputs(n, want, method == "wavefront")
    if offs is None:
        stride = 0
    a, offs = _lighting_args(n_samples, light_radius, offs, stride, base, lib)
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    if method == "recursive":
        rc = lib.rt_trace_rays_soft_recursive(buf, len(blob), C.byref(a), C.c_void_p(offs.ctypes.data), levels, n, C.c_void_p(aligned.ctypes.data), segs,
                                              1 if order == "binned" else 0, C.byref(bufs), None)
        _check(lib, rc, "rt_trace_rays_soft_recursive")
        return out
    counts = np.zeros(RT_MAX_SEGS, np.uint64)
    rc = lib.rt_trace_rays_soft(buf, len(blob), C.byref(a), C.c_void_p(offs.ctypes.data), levels, n, C.c_void_p(aligned.ctypes.data), segs,
                                1 if order_levels else 0, C.byref(bufs), None, counts.ctypes.data_as(C.POINTER(C.c_uint64)))
    _check(lib, rc, "rt_trace_rays_soft")
    if "level_counts" in want:
        out["level_counts"] = counts
    return out


def trace_view_soft(scene, v, w, h, n_samples, light_radius, offs=None, stride=1, levels=1, segs=0, order_levels=False, want=("rgba",), lib=None,
                    method="wavefront"):
    """trace_rays_soft of what the view sees at w x h, in frame order ("rgba" (w h, 4) uint8 is the frame).
    method "wavefront" (the default): the rays are made on the HOST (view_rays, the generator's restatement), cross the link at 48 bytes
    each and go through the wavefront loop.  method "recursive": the view's rays are generated on the GPU and traced there, one launch
    per chunk of whole rows (rt_trace_view_soft) - only the offset table goes up and the frame comes back; the same bytes."""
    if method not in ("wavefront", "recursive"):
        raise ValueError("method is 'wavefront' or 'recursive'")
    if method == "wavefront":
        return trace_rays_soft(scene, view_rays(v, w, h, lib=lib), n_samples, light_radius, offs=offs, stride=stride, levels=levels, segs=segs,
                               order_levels=order_levels, want=want, lib=lib)
    if order_levels:
        raise ValueError("order_levels is the wavefront method's")
    if levels < 0 or levels >= 2 ** 32:
        raise ValueError("levels is a count of levels, 0 .. 2^32 - 1")
    lib = lib or load_library()
    blob = scene if isinstance(scene, (bytes, bytearray)) else flatten_scene(scene)
    want, out, bufs = _soft_outputs(max(int(w) * int(h), 0), want, False)
    if offs is None:
        stride = 0
    a, offs = _lighting_args(n_samples, light_radius, offs, stride, 0, lib)
    _init_once(lib)
    buf = C.create_string_buffer(blob, len(blob))
    rc = lib.rt_trace_view_soft(buf, len(blob), C.byref(v), w, h, C.byref(a), C.c_void_p(offs.ctypes.data), levels, segs, C.byref(bufs), None)
    _check(lib, rc, "rt_trace_view_soft")
    return out


def _jsmin(a, b):
    import numpy as np
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(a < b, a, b))


def _jsmax(a, b):
    import numpy as np
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(a > b, a, b))


def fold_nodes_host(nodes, links, child_rgb):
    """The fold of Renderer.fold_nodes in numpy, operation for operation (main.js:322-336): nodes (NODE_DTYPE, n), links ((n, 2) int32,
    or None = the deepest level), child_rgb ((m, 3) float64) -> (n, 3) float64.  A miss keeps its sample; otherwise per channel
    max(sample * ambient, min(1, sample * diffuse + sample * specular + re + rf)), the terms added left to right, re / rf the linked
    child's colour times reflect_weight / refract_weight or +0.0, Math.min / Math.max with JavaScript's NaN rule."""
    import numpy as np
    nodes = np.asarray(nodes)
    n = nodes.shape[0]
    s = nodes["sample"].astype(np.float64)
    re, rf = np.zeros((n, 3)), np.zeros((n, 3))
    if links is not None:
        links = np.asarray(links).reshape(n, 2)
        child_rgb = np.asarray(child_rgb, np.float64).reshape(-1, 3)
        for k, (dst, w) in enumerate(((re, nodes["reflect_weight"]), (rf, nodes["refract_weight"]))):
            m = links[:, k] >= 0
            dst[m] = child_rgb[links[m, k]] * w[m, None]
    with np.errstate(invalid="ignore", over="ignore"):
        shade = s * nodes["diffuse"][:, None] + s * nodes["specular"][:, None] + re + rf
        out = _jsmax(s * nodes["ambient"][:, None], _jsmin(np.float64(1.0), shade))
    miss = nodes["object"] < 0
    out[miss] = s[miss]
    return out
