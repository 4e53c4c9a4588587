"""numpy / ctypes mirrors of include/zelda_abi.h (the ZeldaEngine submission structs).

Reference layouts: XkVertex ZE:417-422, XkInstanceData ZE:409-414, XkMeshlet ZE:689-701,
XkLight ZE:772-787, XkUniformBufferMVP ZE:384-388, XkView ZE:922-940
(ZE = Engine/ZeldaEngine/ZeldaEngine.cpp).
"""
import ctypes as C

import numpy as np

MAX_DIRECTIONAL_LIGHTS = 16
MAX_POINT_LIGHTS = 512
MAX_SPOT_LIGHTS = 16
SHADOWMAP_DIM = 1024
TILE = 32

XkVertex = np.dtype([("Position", "<f4", 3), ("Normal", "<f4", 3), ("Color", "<f4", 3), ("TexCoord", "<f4", 2)])
XkInstanceData = np.dtype([("InstancePosition", "<f4", 3), ("InstanceRotation", "<f4", 3), ("InstancePScale", "<f4"),
                           ("InstanceTexIndex", "u1"), ("_pad", "u1", 3)])
XkMeshlet = np.dtype([("VertexOffset", "<u4"), ("VertexCount", "<u4"), ("TriangleOffset", "<u4"), ("TriangleCount", "<u4"),
                      ("BoundsCenter", "<f4", 3), ("BoundsRadius", "<f4"), ("ConeApex", "<f4", 3), ("ConeAxis", "<f4", 3),
                      ("ConeCutoff", "<f4"), ("BindlessContext", "<u4")])
XkMeshletFileVertex = np.dtype([("pos", "<f4", 3), ("nrm", "<f4", 3), ("uv", "<f4", 2)])
XkLight = np.dtype([("Position", "<f4", 4), ("Color", "<f4", 4), ("Direction", "<f4", 4), ("LightInfo", "<f4", 4)])
XkUniformBufferMVP = np.dtype([("Model", "<f4", 16), ("View", "<f4", 16), ("Proj", "<f4", 16)])
XkView = np.dtype([("ViewProjSpace", "<f4", 16), ("ShadowmapSpace", "<f4", 16), ("LocalToWorld", "<f4", 16),
                   ("CameraInfo", "<f4", 4), ("ViewportInfo", "<f4", 4),
                   ("DirectionalLights", XkLight, MAX_DIRECTIONAL_LIGHTS), ("PointLights", XkLight, MAX_POINT_LIGHTS),
                   ("SpotLights", XkLight, MAX_SPOT_LIGHTS), ("LightsCount", "<i4", 4),
                   ("Time", "<f4"), ("zNear", "<f4"), ("zFar", "<f4")])

assert XkVertex.itemsize == 44 and XkInstanceData.itemsize == 32 and XkMeshlet.itemsize == 64
assert XkLight.itemsize == 64 and XkUniformBufferMVP.itemsize == 192 and XkView.itemsize == 35068


class Image(C.Structure):
    _fields_ = [("rgba8", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32)]


class Material(C.Structure):
    _fields_ = [("tex", Image * 7)]


TEXTURE_SLOTS = ("bc", "m", "r", "n", "ao", "ev", "ms")      # the material's slots in order (zr_material::tex, zr_object_set_texture)
# the texture-update entries of include/zelda_render.h (engine.lib() binds them with the rest)
vp_, u32_ = C.c_void_p, C.c_uint32
TEXTURE_UPDATE_SIGNATURES = {
    "zr_object_set_texture": [vp_, u32_, u32_, C.POINTER(Image)],
    "zr_object_update_texture_async": [vp_, u32_, u32_, vp_, u32_, u32_, vp_],
    "zr_object_get_texture": [vp_, u32_, u32_, u32_, vp_, C.c_size_t, C.POINTER(u32_), C.POINTER(u32_), C.POINTER(u32_)],
}
# hiding and showing (include/zelda_render.h, "Hiding and showing"); merged into engine.lib()'s table like the texture block
VISIBILITY_SIGNATURES = {
    "zr_object_set_visible": [vp_, u32_, C.c_int],
    "zr_object_set_instance_visibility": [vp_, u32_, u32_, vp_, u32_],
    "zr_object_update_instance_visibility_async": [vp_, u32_, u32_, vp_, vp_, u32_, vp_],
    "zr_object_get_visibility": [vp_, u32_, C.POINTER(C.c_int), vp_, C.POINTER(u32_)],
}
# delivering changes (include/zelda_render.h, "delivering changes")
FRAME_DELTA_SIGNATURES = {
    "zr_set_frame_delta": [vp_, C.c_int],
    "zr_frame_delta_reset": [vp_],
    "zr_read_frame_delta": [vp_, vp_, u32_, vp_, C.c_size_t, vp_, C.c_size_t],
    "zr_copy_frame_delta_async": [vp_, vp_, vp_, vp_],
    "zr_read_frame_delta_packed": [vp_, vp_, u32_, vp_, u32_, vp_, C.c_size_t, vp_, C.c_size_t],
    "zr_copy_frame_delta_packed_async": [vp_, vp_, vp_, vp_, vp_],
    "zr_frame_delta_decode": [vp_, vp_, u32_, vp_, C.c_size_t, u32_, u32_, vp_],
}
# delivering a scaled frame (include/zelda_render.h, "delivering a scaled frame")
FRAME_SCALE_SIGNATURES = {
    "zr_frame_scaled_extent": [u32_, u32_, u32_, C.POINTER(u32_), C.POINTER(u32_)],
    "zr_frame_downscale": [vp_, u32_, u32_, u32_, vp_, C.c_size_t],
    "zr_read_color_scaled": [vp_, u32_, vp_, C.c_size_t],
    "zr_copy_frame_scaled_async": [vp_, u32_, vp_],
    "zr_set_frame_delta_scale": [vp_, u32_],
    "zr_get_frame_delta_extent": [vp_, C.POINTER(u32_), C.POINTER(u32_), C.POINTER(u32_), C.POINTER(u32_)],
}
FRAME_SCALE_MAX = 8               # the largest factor of the scaled forms


class HighlightStyle(C.Structure):
    """ctypes mirror of zr_highlight_style (16 bytes, passed with its size, like zr_stats)"""
    _fields_ = [("outline", C.c_uint8 * 4), ("fill", C.c_uint8 * 4), ("radius", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(HighlightStyle) == 16
HIGHLIGHT_RADIUS_MAX = 8          # the widest outline
# highlighting a selection (include/zelda_render.h, "highlighting a selection")
HIGHLIGHT_SIGNATURES = {
    "zr_highlight_set": [vp_, u32_, u32_, vp_, u32_],
    "zr_highlight_clear": [vp_],
    "zr_highlight_get": [vp_, vp_, C.c_size_t],
    "zr_set_highlight_style": [vp_, C.POINTER(HighlightStyle), C.c_size_t],
    "zr_get_highlight_style": [vp_, C.POINTER(HighlightStyle), C.c_size_t],
    "zr_read_color_highlighted": [vp_, u32_, vp_, C.c_size_t],
    "zr_copy_frame_highlighted_async": [vp_, u32_, vp_],
    "zr_set_frame_delta_highlight": [vp_, C.c_int],
    "zr_frame_highlight": [vp_, vp_, u32_, u32_, C.POINTER(HighlightStyle), C.c_size_t, vp_, C.c_size_t],
}


class OverlaySegment(C.Structure):
    """ctypes mirror of zr_overlay_segment (32 bytes)"""
    _fields_ = [("a", C.c_float * 3), ("b", C.c_float * 3), ("rgba", C.c_uint8 * 4), ("flags", C.c_uint32)]


class OverlayStyle(C.Structure):
    """ctypes mirror of zr_overlay_style (16 bytes, passed with its size, like zr_stats)"""
    _fields_ = [("depth_bias", C.c_float), ("hidden_opacity", C.c_uint32), ("reserved", C.c_uint32 * 2)]


assert C.sizeof(OverlaySegment) == 32 and C.sizeof(OverlayStyle) == 16
# numpy mirror of zr_overlay_segment: what Renderer.overlay_set takes and overlay_get returns
OVERLAY_SEGMENT = np.dtype([("a", "<f4", 3), ("b", "<f4", 3), ("rgba", "u1", 4), ("flags", "<u4")])
assert OVERLAY_SEGMENT.itemsize == 32
OVERLAY_XRAY = 1                  # ZR_OVERLAY_XRAY: the segment is not depth-tested
OVERLAY_MAX_SEGMENTS = 16384
# overlaying lines (include/zelda_render.h, "overlaying lines")
OVERLAY_SIGNATURES = {
    "zr_overlay_set": [vp_, vp_, u32_],
    "zr_overlay_get": [vp_, vp_, C.POINTER(u32_)],
    "zr_set_overlay_style": [vp_, C.POINTER(OverlayStyle), C.c_size_t],
    "zr_get_overlay_style": [vp_, C.POINTER(OverlayStyle), C.c_size_t],
    "zr_read_color_overlaid": [vp_, u32_, C.c_int, vp_, C.c_size_t],
    "zr_copy_frame_overlaid_async": [vp_, u32_, C.c_int, vp_],
    "zr_set_frame_delta_overlay": [vp_, C.c_int],
    "zr_frame_overlay": [vp_, vp_, u32_, u32_, vp_, vp_, u32_, C.POINTER(OverlayStyle), C.c_size_t, vp_, C.c_size_t],
}


class WireStyle(C.Structure):
    """ctypes mirror of zr_wire_style (16 bytes, passed with its size, like zr_stats)"""
    _fields_ = [("rgba", C.c_uint8 * 4), ("width_256", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


# numpy mirror of zr_wire_style
WIRE_STYLE = np.dtype([("rgba", "u1", 4), ("width_256", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
assert C.sizeof(WireStyle) == WIRE_STYLE.itemsize == 16
WIRE_SELECTED = 1                 # ZR_WIRE_SELECTED: only the instances of the highlight set
WIRE_WIDTH_MAX = 4096             # ZR_WIRE_WIDTH_MAX: the widest line, in 1/256 pixel
STAGE_WIRE, STAGE_HIGHLIGHT, STAGE_OVERLAY = 1, 2, 4         # ZR_STAGE_*: the stages of a staged delivery, applied in this order
# the wireframe (include/zelda_render.h, "wireframe")
WIRE_SIGNATURES = {
    "zr_set_wire_style": [vp_, C.POINTER(WireStyle), C.c_size_t],
    "zr_get_wire_style": [vp_, C.POINTER(WireStyle), C.c_size_t],
    "zr_read_color_staged": [vp_, u32_, u32_, vp_, C.c_size_t],
    "zr_copy_frame_staged_async": [vp_, u32_, u32_, vp_],
    "zr_set_frame_delta_wire": [vp_, C.c_int],
    "zr_frame_wire": [vp_, vp_, u32_, u32_, vp_, u32_, vp_, C.POINTER(WireStyle), C.c_size_t, vp_, C.c_size_t],
}
# zr_get_rest_settled / zr_get_rest_settled_parts: the parts a resting frame's launch left as they stand (a count; a byte per part)
REST_SETTLE_SIGNATURES = {
    "zr_get_rest_settled": [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)],
    "zr_get_rest_settled_parts": [C.c_void_p, C.c_void_p, C.c_size_t],
}
# casting rays (include/zelda_render.h, "casting rays"): numpy mirrors of zr_ray / zr_ray_hit - what Renderer.raycast takes and returns
RAY = np.dtype([("origin", "<f4", 3), ("t_min", "<f4"), ("dir", "<f4", 3), ("t_max", "<f4")])
RAY_RECORD = np.dtype([("object", "<u4"), ("instance", "<u4"), ("triangle", "<u4"), ("flags", "<u4"), ("t", "<f4"), ("u", "<f4"), ("v", "<f4"),
                    ("reserved", "<u4"), ("normal", "<f4", 3), ("reserved2", "<u4")])


class Ray(C.Structure):
    """ctypes mirror of zr_ray (32 bytes)"""
    _fields_ = [("origin", C.c_float * 3), ("t_min", C.c_float), ("dir", C.c_float * 3), ("t_max", C.c_float)]


class RayHit(C.Structure):
    """ctypes mirror of zr_ray_hit (48 bytes)"""
    _fields_ = [("object", C.c_uint32), ("instance", C.c_uint32), ("triangle", C.c_uint32), ("flags", C.c_uint32), ("t", C.c_float), ("u", C.c_float),
                ("v", C.c_float), ("reserved", C.c_uint32), ("normal", C.c_float * 3), ("reserved2", C.c_uint32)]


assert RAY.itemsize == C.sizeof(Ray) == 32 and RAY_RECORD.itemsize == C.sizeof(RayHit) == 48
RAY_HIT_FLAG, RAY_HIT_BACK, RAY_INVALID = 1, 2, 4            # ZR_RAY_HIT, ZR_RAY_HIT_BACK, ZR_RAY_INVALID: RayHit.flags
RAY_CULL_BACK, RAY_ANY_HIT, RAY_NO_BOUNDS = 1, 2, 4          # ZR_RAY_CULL_BACK, ZR_RAY_ANY_HIT, ZR_RAY_NO_BOUNDS: the query's flags
RAY_MAX_RAYS = 1 << 24
RAYCAST_SIGNATURES = {
    "zr_raycast": [vp_, vp_, u32_, u32_, vp_, C.c_size_t],
    "zr_raycast_async": [vp_, vp_, u32_, u32_, vp_],
    "zr_camera_ray": [vp_, C.c_float, C.c_float, C.POINTER(Ray)],
    "zr_ray_triangles": [vp_, u32_, vp_, u32_, u32_, vp_],
}
# the extent of a live context (include/zelda_render.h, "lifetime")
EXTENT_SIGNATURES = {
    "zr_resize": [vp_, u32_, u32_],
    "zr_get_extent": [vp_, C.POINTER(u32_), C.POINTER(u32_)],
}
del vp_, u32_


def make_highlight_style(outline=(255, 160, 0, 255), fill=(255, 160, 0, 0), radius=2):
    """zr_highlight_style from (R, G, B, opacity) tuples and the outline's width; the defaults are the library's"""
    return HighlightStyle((C.c_uint8 * 4)(*outline), (C.c_uint8 * 4)(*fill), radius, 0)


def make_wire_style(rgba=(0, 0, 0, 255), width_256=256, flags=0):
    """zr_wire_style from an (R, G, B, opacity) tuple, the full line width in 1/256 pixel and WIRE_SELECTED or 0; the defaults are the library's"""
    return WireStyle((C.c_uint8 * 4)(*rgba), width_256, flags, 0)


def make_rays(origins, dirs, t_min=0.0, t_max=np.inf):
    """A RAY array from (n, 3) origins and directions and bounds (scalars or (n,) arrays)"""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(len(o), dtype=RAY)
    out["origin"], out["dir"] = o, np.asarray(dirs, dtype=np.float32).reshape(-1, 3)
    out["t_min"], out["t_max"] = t_min, t_max
    return out


def make_overlay_style(depth_bias=0.0, hidden_opacity=0):
    """zr_overlay_style; the defaults are the library's"""
    return OverlayStyle(depth_bias, hidden_opacity, (C.c_uint32 * 2)(0, 0))


def make_overlay_segments(segments):
    """An OVERLAY_SEGMENT array from one, or from rows (ax, ay, az, bx, by, bz, r, g, b, a[, flags])"""
    if isinstance(segments, np.ndarray) and segments.dtype == OVERLAY_SEGMENT:
        return np.ascontiguousarray(segments).reshape(-1)
    rows = [tuple(s) for s in segments]
    out = np.zeros(len(rows), dtype=OVERLAY_SEGMENT)
    for i, s in enumerate(rows):
        out[i]["a"], out[i]["b"], out[i]["rgba"], out[i]["flags"] = s[0:3], s[3:6], s[6:10], s[10] if len(s) > 10 else 0
    return out


class Camera(C.Structure):
    _fields_ = [("Position", C.c_float * 3), ("Lookat", C.c_float * 3), ("Speed", C.c_float), ("FOV", C.c_float),
                ("zNear", C.c_float), ("zFar", C.c_float)]


class Config(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("shadow_dim", C.c_uint32), ("debug_view", C.c_uint32),
                ("device", C.c_int32), ("tile_rank", C.c_uint32), ("tile_world", C.c_uint32), ("flags", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("work_items", C.c_uint64 * 2), ("survivors", C.c_uint64 * 2), ("bin_entries", C.c_uint64 * 2),
                ("covered_pixels", C.c_uint64), ("covered_shadow_texels", C.c_uint64), ("overflow", C.c_uint32), ("hiz_culled", C.c_uint32),
                ("round1_survivors", C.c_uint64), ("shadow_occluded", C.c_uint32), ("shadow_late", C.c_uint32),
                ("hiz_culled_geom", C.c_uint32), ("struct_bytes", C.c_uint32)]


class LightKeep(C.Structure):
    """ctypes mirror of zr_light_keep: what the lighting passes did with the plane of standing terms (passed with its size, like zr_stats)"""
    _fields_ = [("last", C.c_uint32), ("_pad", C.c_uint32), ("ignored", C.c_uint64), ("filled", C.c_uint64), ("read", C.c_uint64),
                ("plane_bytes", C.c_uint64), ("read_by_arg", C.c_uint64)]


LIGHT_PLANE_IGNORED, LIGHT_PLANE_FILLED, LIGHT_PLANE_READ = 0, 1, 2      # ZR_LIGHT_PLANE_*: LightKeep.last


class WorldDelta(C.Structure):
    """ctypes mirror of zr_world_delta: what zr_world_update_json did (passed with its size, like zr_stats)"""
    _fields_ = [("struct_bytes", C.c_uint32), ("differs", C.c_uint32), ("scene_changed", C.c_uint32), ("objects_kept", C.c_uint32),
                ("objects_reinstanced", C.c_uint32), ("objects_added", C.c_uint32), ("objects_removed", C.c_uint32),
                ("materials_rebuilt", C.c_uint32), ("history_items", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class FrameDelta(C.Structure):
    """ctypes mirror of zr_frame_delta: the 16-byte header of a delivery (passed with its size, like zr_stats)"""
    _fields_ = [("n_tiles", C.c_uint32), ("total_tiles", C.c_uint32), ("full", C.c_uint32), ("serial", C.c_uint32)]


class FrameDeltaPacked(C.Structure):
    """ctypes mirror of zr_frame_delta_packed: the 32-byte header of a packed delivery (passed with its size, like zr_stats)"""
    _fields_ = FrameDelta._fields_ + [("bytes", C.c_uint32), ("raw_tiles", C.c_uint32), ("reserved", C.c_uint32 * 2)]


assert C.sizeof(FrameDelta) == 16 and C.sizeof(FrameDeltaPacked) == 32
TILE_BYTES = TILE * TILE * 4      # one slot of a delivery
FRAME_DELTA_PACKED = 3            # ZR_FRAME_DELTA_PACKED: zr_set_frame_delta's value that enables the packed forms as well
RECORD_MAX_BYTES = 8 + TILE_BYTES      # ZR_FRAME_DELTA_RECORD_MAX: the longest record of a packed delivery

# ZR_WORLD_DIFF_*: the bits of WorldDelta.differs and of engine.world_json_diff
WORLD_DIFF_CAMERA, WORLD_DIFF_LIGHTS, WORLD_DIFF_SKY, WORLD_DIFF_BACKGROUND, WORLD_DIFF_OBJECTS = 1, 2, 4, 8, 16

ABI_VERSION = 7      # ZR_ABI_VERSION of include/zelda_render.h

# object identity of the last frame (zr_read_ids / zr_pick)
IDS_PRIMITIVE = 0     # ZR_IDS_PRIMITIVE: (H, W) uint32 global draw-order primitive id, 0xFFFFFFFF = none
IDS_OBJECT = 1        # ZR_IDS_OBJECT: (H, W, 2) uint32 {object (add order), instance}, all ones = none
NO_ID = 0xFFFFFFFF
Hit = np.dtype([("object", "<u4"), ("instance", "<u4"), ("pixels", "<u4"), ("triangle", "<u4"), ("x", "<u4"), ("y", "<u4"),
                ("depth", "<f4"), ("reserved", "<u4")])


class HitC(C.Structure):
    """ctypes mirror of zr_hit (the same 32 bytes as Hit)"""
    _fields_ = [("object", C.c_uint32), ("instance", C.c_uint32), ("pixels", C.c_uint32), ("triangle", C.c_uint32),
                ("x", C.c_uint32), ("y", C.c_uint32), ("depth", C.c_float), ("reserved", C.c_uint32)]


assert Hit.itemsize == 32 and C.sizeof(HitC) == 32


PASS_NAMES = ["cull_shadow", "shadow", "cull_camera", "gbuffer", "hiz", "gbuffer2", "resolve", "lighting", "composite", "total"]
GBUFFER_DTYPES = [np.dtype("<f4"), np.dtype("<u4"), np.dtype("<u4"), np.dtype("<u4"), np.dtype("<u4"), np.dtype("<u8")]

FLAG_NO_FRUSTUM_CULL = 1
FLAG_NO_CONE_CULL = 2
FLAG_SKIP_COMPOSITE = 4
FLAG_NO_HIZ = 8
FLAG_SERIAL_PASSES = 16
FLAG_PACKED_TILES = 32
FLAG_NO_RECT_CULL = 64
FLAG_MESHLET_BINS = 128
FLAG_NO_LIST_REUSE = 256
FLAG_NO_SHADOW_OCCLUSION = 512
FLAG_SHADOW_OCCLUSION = 1024

OK, ERR_ARG, ERR_DEVICE, ERR_OOM, ERR_PARSE, ERR_IO, ERR_STATE, ERR_OVERFLOW, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6, -7, -8


def make_light(position=(0, 0, 0), type_=0, color=(1, 1, 1), intensity=1.0, direction=(0, 0, 1), radius=0.0,
               extra=(0, 0, 0, 0)):
    """XkLight(const XkLightDesc&), ZE:781-787."""
    l = np.zeros((), dtype=XkLight)
    l["Position"] = (*position, float(type_))
    l["Color"] = (*color, intensity)
    l["Direction"] = (*direction, radius)
    l["LightInfo"] = extra
    return l


def make_camera(position=(5.0, 5.0, 5.0), lookat=(0.0, 0.0, 0.0), speed=2.5, fov=45.0, znear=0.1, zfar=45.0):
    """XkCameraDesc defaults, ZE:882-887."""
    return Camera((C.c_float * 3)(*position), (C.c_float * 3)(*lookat), speed, fov, znear, zfar)


def make_material(images=None):
    """images: list of 7 entries, each None (engine default) or an (H, W, 4) uint8 array.  Returns (Material, keepalive)."""
    m = Material()
    keep = []
    for i in range(7):
        img = images[i] if images else None
        if img is None:
            m.tex[i] = Image(None, 0, 0)
        else:
            a = np.ascontiguousarray(img, dtype=np.uint8)
            assert a.ndim == 3 and a.shape[2] == 4
            keep.append(a)
            m.tex[i] = Image(a.ctypes.data, a.shape[1], a.shape[0])
    return m, keep


DIST_SPLIT_SHADOW = 1      # ZR_DIST_SPLIT_SHADOW: casters i % world == rank + ncclAllReduce(min) of the maps
DIST_SHADOW_TILES = 2      # ZR_DIST_SHADOW_TILES: the map owned by light-space super-tiles + ncclAllGather of the packed tiles
SHADOW_MODES = ("replicated", "split", "tiles")


def shadow_mode(split_shadow=False, mode=None):
    """The multi-GPU shadow mode from the two ways hosts name it: mode in SHADOW_MODES, or the older split_shadow flag."""
    if mode is None:
        mode = "split" if split_shadow is True else (split_shadow if isinstance(split_shadow, str) else "replicated")
    if mode not in SHADOW_MODES:
        raise ValueError("shadow mode %r: one of %r" % (mode, SHADOW_MODES))
    return mode


def dist_flags(mode):
    return {"replicated": 0, "split": DIST_SPLIT_SHADOW, "tiles": DIST_SHADOW_TILES}[mode]
