"""ctypes binding of libzelda_render.so — the HIP renderer behind the C-ABI of include/zelda_render.h.

`Renderer` mirrors the call sequence of XkZeldaEngineApp (ZE = Engine/ZeldaEngine/ZeldaEngine.cpp):
CreateEngineScene (ZE:4140) -> mesh_create / object_add, UpdateUniformBuffer (ZE:4585) -> update_uniforms,
DrawFrame (ZE:1940) -> render, plus read-back in place of the swapchain.

There is no CPU path here: the library fails loudly when the HIP extension or a GPU is missing.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZELDA_RENDER_LIB") or os.path.join(_HERE, "libzelda_render.so")   # env: A/B builds only

_lib = None


class ZeldaRenderError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("zelda_render error %d: %s" % (code, msg))
        self.code = code


def lib():
    """Loads the in-tree shared library (built by zeldaengine_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libzelda_render.so is not built: run `python -m zeldaengine_amd.build` "
                          "(hipcc --offload-arch=gfx950); there is no fallback path")
    try:
        import torch  # noqa: F401  -- first, so that this process has ONE HIP runtime (torch's bundled libamdhip64.so)
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    sig = {
        "zr_create": [C.POINTER(abi.Config), C.POINTER(vp)],
        "zr_set_stream": [vp, vp],
        "zr_mesh_create": [vp, vp, u32, vp, u32, C.POINTER(u32)],
        "zr_mesh_set_meshlets": [vp, u32, vp, u32, vp, sz, vp, sz],
        "zr_mesh_build_meshlets": [vp, u32, u32, u32, C.c_float],
        "zr_mesh_get_meshlets": [vp, u32, vp, C.POINTER(u32), vp, C.POINTER(sz), vp, C.POINTER(sz)],
        "zr_meshlets_build": [vp, u32, vp, u32, u32, u32, C.c_float, vp, C.POINTER(u32), vp, C.POINTER(sz), vp, C.POINTER(sz), vp],
        "zr_object_add": [vp, u32, vp, vp, u32],
        "zr_scene_clear": [vp],
        "zr_set_limits": [vp, u32, u32],
        "zr_set_bucket_share": [vp, u32],
        "zr_object_count": [vp, C.POINTER(u32)],
        "zr_object_get_instances": [vp, u32, C.POINTER(u32), vp, C.POINTER(u32)],
        "zr_object_set_instances": [vp, u32, u32, vp, u32],
        "zr_object_update_instances_async": [vp, u32, u32, vp, vp, u32, vp],
        "zr_mesh_set_vertices": [vp, u32, u32, vp, u32],
        "zr_mesh_update_vertices_async": [vp, u32, u32, vp, u32, vp],
        "zr_mesh_get_vertices": [vp, u32, vp, C.POINTER(u32)],
        **abi.TEXTURE_UPDATE_SIGNATURES,
        **abi.VISIBILITY_SIGNATURES,
        **abi.FRAME_DELTA_SIGNATURES,
        **abi.FRAME_SCALE_SIGNATURES,
        **abi.HIGHLIGHT_SIGNATURES,
        **abi.OVERLAY_SIGNATURES,
        **abi.WIRE_SIGNATURES,
        **abi.EXTENT_SIGNATURES,
        **abi.RAYCAST_SIGNATURES,
        **abi.REST_SETTLE_SIGNATURES,
        "zr_set_cubemap": [vp, vp, u32],
        "zr_set_skydome": [vp, vp, u32, vp, u32, vp],
        "zr_set_background": [vp, vp],
        "zr_set_sky_flags": [vp, C.c_int, C.c_int],
        "zr_update_uniforms": [vp, vp, vp, u32, vp, u32, vp, u32, C.c_float, C.c_float, C.c_float],
        "zr_set_frame": [vp, vp, vp, vp],
        "zr_get_frame": [vp, vp, vp, vp],
        "zr_set_debug_view": [vp, u32],
        "zr_set_shading": [vp, u32],
        "zr_render": [vp],
        "zr_render_shadow": [vp], "zr_render_gbuffer": [vp], "zr_render_lighting": [vp],
        "zr_render_geometry": [vp], "zr_stream_wait_shadow": [vp, vp],
        "zr_set_shadow_partition": [vp, u32, u32], "zr_set_shadow_buffer": [vp, vp],
        "zr_set_shadow_tiles": [vp, u32, u32], "zr_shadow_tiles_bytes": [vp, C.POINTER(sz)],
        "zr_shadow_pack": [vp, vp, vp], "zr_shadow_unpack": [vp, vp, vp],
        "zr_finish": [vp],
        "zr_get_pass_times": [vp, vp],
        "zr_get_pass_times_avg": [vp, u32, vp],
        "zr_set_timing_interval": [vp, u32],
        "zr_get_frame_latencies": [vp, u32, vp],
        "zr_get_frame_periods": [vp, u32, vp],
        "zr_get_stats": [vp, C.POINTER(abi.Stats), sz],
        "zr_get_light_keep": [vp, C.POINTER(abi.LightKeep), sz],
        "zr_read_color": [vp, vp, sz],
        "zr_read_gbuffer": [vp, C.c_int, vp, sz],
        "zr_read_shadowmap": [vp, vp, sz],
        "zr_copy_frame_async": [vp, vp, vp],
        "zr_set_id_capture": [vp, C.c_int],
        "zr_read_ids": [vp, C.c_int, vp, sz],
        "zr_pick": [vp, u32, u32, u32, u32, vp, u32, C.POINTER(u32)],
        "zr_instance_coverage": [vp, vp, sz],
        "zr_instance_coverage_async": [vp, vp, sz],
        "zr_tiles_device_buffer": [vp, C.POINTER(vp), C.POINTER(sz)],
        "zr_composite": [vp, vp],
        "zr_read_tiles": [vp, vp, sz],
        "zr_set_tiles_buffer": [vp, vp],
        "zr_tile_size": [],
        "zr_color_device_ptr": [vp, C.POINTER(vp)],
        "zr_tile_partition": [u32, u32, u32, u32, vp, C.POINTER(u32), C.POINTER(u32)],
        "zr_dist_unique_id": [vp, sz],
        "zr_dist_init": [vp, vp, sz, u32, u32, u32],
        "zr_dist_prepare": [vp, u32, u32, u32],
        "zr_dist_connect": [vp, vp, sz],
        "zr_dist_frame": [vp],
        "zr_dist_copy_frame_async": [vp, vp],
        "zr_profab_register": [vp, C.c_char_p, u32, vp],
        "zr_world_load_json": [vp, C.c_char_p, sz],
        "zr_set_asset_root": [vp, C.c_char_p],
        "zr_asset_path_search": [vp, C.c_char_p, vp, sz, C.POINTER(sz)],
        "zr_load_obj": [C.c_char_p, vp, C.POINTER(u32), vp, C.POINTER(u32)],
        "zr_load_png_rgba8": [C.c_char_p, vp, sz, C.POINTER(u32), C.POINTER(u32)],
        "zr_load_meshlet_file": [vp, C.c_char_p, C.POINTER(u32)],
        "zr_world_load_file": [vp, C.c_char_p],
        "zr_world_save_file": [vp, C.c_char_p],
        "zr_world_update_uniforms": [vp, C.c_float, C.c_float, C.c_float],
        "zr_world_save_json": [vp, vp, sz, C.POINTER(sz)],
        "zr_world_get_camera": [vp, vp],
        "zr_world_json_normalize": [C.c_char_p, sz, vp, sz, C.POINTER(sz)],
        "zr_livelink_bind_any": [vp, C.c_int],
        "zr_livelink_serve": [vp, C.c_uint16],
        "zr_livelink_port": [vp, C.POINTER(C.c_uint16)],
        "zr_livelink_poll": [vp, C.POINTER(C.c_int)],
        "zr_livelink_stop": [vp],
        "zr_world_update_json": [vp, C.c_char_p, sz, C.POINTER(abi.WorldDelta), sz],
        "zr_world_update_file": [vp, C.c_char_p, C.POINTER(abi.WorldDelta), sz],
        "zr_world_json_diff": [C.c_char_p, sz, C.c_char_p, sz, C.POINTER(u32)],
        "zr_livelink_set_incremental": [vp, C.c_int],
    }
    for name, args in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = C.c_int
    L.zr_abi_version.argtypes = []
    L.zr_abi_version.restype = u32
    if L.zr_abi_version() != abi.ABI_VERSION:
        raise ImportError("libzelda_render.so speaks ABI version %d, this binding %d: rebuild (python -m zeldaengine_amd.build --force)"
                          % (L.zr_abi_version(), abi.ABI_VERSION))
    L.zr_tile_owner.argtypes = [u32, u32, u32]
    L.zr_tile_owner.restype = u32
    L.zr_destroy.argtypes = [vp]
    L.zr_destroy.restype = None
    L.zr_last_error.argtypes = [vp]
    L.zr_last_error.restype = C.c_char_p
    _lib = L
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _addr(a):
    return a.ctypes.data if a is not None and a.size else None


def uniform_arguments(cam, dir_l, point_l, spot_l):
    """zr_update_uniforms' pointer and count arguments as plain integers (None: a null pointer), read from the objects at every call: no
    pointer object, no cast and no kept address that an array's reallocation or another camera object could leave stale.  An empty
    array or None goes as a null pointer and a count of 0.  Needs no GPU (tests/test_uniform_marshalling.py)."""
    return (C.addressof(cam), _addr(dir_l), 0 if dir_l is None else len(dir_l), _addr(point_l), 0 if point_l is None else len(point_l),
            _addr(spot_l), 0 if spot_l is None else len(spot_l))


def build_meshlets(verts, idx, max_vertices=64, max_triangles=124, cone_weight=0.2):
    """Context-free clusteriser (host code only; works without a GPU).  Returns (meshlets, mverts, mtris, tri_order)."""
    L = lib()
    verts = np.ascontiguousarray(verts)
    assert verts.dtype == abi.XkVertex
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    nm, nmv, nmt = C.c_uint32(), C.c_size_t(), C.c_size_t()
    args = (_ptr(verts), len(verts), _ptr(idx), len(idx), max_vertices, max_triangles, cone_weight)
    rc = L.zr_meshlets_build(*args, None, C.byref(nm), None, C.byref(nmv), None, C.byref(nmt), None)
    if rc:
        raise ZeldaRenderError(rc, "zr_meshlets_build")
    ml = np.zeros(nm.value, dtype=abi.XkMeshlet)
    mv = np.zeros(nmv.value, dtype=np.uint32)
    mt = np.zeros(nmt.value, dtype=np.uint8)
    order = np.zeros(nmt.value // 3, dtype=np.uint32)
    rc = L.zr_meshlets_build(*args, _ptr(ml), C.byref(nm), _ptr(mv), C.byref(nmv), _ptr(mt), C.byref(nmt), _ptr(order))
    if rc:
        raise ZeldaRenderError(rc, "zr_meshlets_build")
    return ml, mv, mt, order


def load_obj(path):
    """LoadMeshAsset through the library's own OBJ reader (host code only) -> (XkVertex[], uint32 indices)."""
    L = lib()
    nv, ni = C.c_uint32(), C.c_uint32()
    rc = L.zr_load_obj(os.fsencode(path), None, C.byref(nv), None, C.byref(ni))
    if rc:
        raise ZeldaRenderError(rc, "zr_load_obj(%s)" % path)
    v = np.zeros(nv.value, dtype=abi.XkVertex)
    idx = np.zeros(ni.value, dtype=np.uint32)
    rc = L.zr_load_obj(os.fsencode(path), _ptr(v), C.byref(nv), _ptr(idx), C.byref(ni))
    if rc:
        raise ZeldaRenderError(rc, "zr_load_obj(%s)" % path)
    return v, idx


def load_png_rgba8(path):
    """LoadTextureAsset through the library's own PNG reader (host code only) -> (H, W, 4) uint8."""
    L = lib()
    w, h = C.c_uint32(), C.c_uint32()
    rc = L.zr_load_png_rgba8(os.fsencode(path), None, 0, C.byref(w), C.byref(h))
    if rc:
        raise ZeldaRenderError(rc, "zr_load_png_rgba8(%s)" % path)
    out = np.zeros((h.value, w.value, 4), dtype=np.uint8)
    rc = L.zr_load_png_rgba8(os.fsencode(path), _ptr(out), out.nbytes, C.byref(w), C.byref(h))
    if rc:
        raise ZeldaRenderError(rc, "zr_load_png_rgba8(%s)" % path)
    return out


def tile_partition(width, height, world, rank):
    """The library's own statement of the multi-GPU tile ownership (host code only) -> (owned tile indices, slots_per_rank)."""
    L = lib()
    n, spr = C.c_uint32(), C.c_uint32()
    rc = L.zr_tile_partition(width, height, world, rank, None, C.byref(n), C.byref(spr))
    if rc:
        raise ZeldaRenderError(rc, "zr_tile_partition")
    owned = np.zeros(n.value, dtype=np.uint32)
    L.zr_tile_partition(width, height, world, rank, _ptr(owned), C.byref(n), C.byref(spr))
    return owned, spr.value


def dist_unique_id():
    """ncclGetUniqueId through the library (128 bytes); rank 0 makes it, every rank passes it to Renderer.dist_init."""
    buf = C.create_string_buffer(128)
    rc = lib().zr_dist_unique_id(buf, 128)
    if rc:
        raise ZeldaRenderError(rc, "zr_dist_unique_id (librccl not loadable?)")
    return buf.raw


def world_json_normalize(text):
    """Context-free XkWorld Load -> Save (host code only).  Raises ZeldaRenderError(ZR_ERR_PARSE) with the loader's message."""
    L = lib()
    b = text.encode() if isinstance(text, str) else bytes(text)
    n = C.c_size_t()
    L.zr_world_json_normalize(b, len(b), None, 0, C.byref(n))
    buf = C.create_string_buffer(max(1, n.value))
    rc = L.zr_world_json_normalize(b, len(b), buf, n.value, C.byref(n))
    out = buf.raw[:n.value].decode(errors="replace")
    if rc:
        raise ZeldaRenderError(rc, out)
    return out


def world_json_diff(a, b):
    """Context-free: which parts of two world payloads differ, as abi.WORLD_DIFF_* bits (host code only).  A malformed payload raises
    ZeldaRenderError(ZR_ERR_PARSE)."""
    L = lib()
    ba = a.encode() if isinstance(a, str) else bytes(a)
    bb = b.encode() if isinstance(b, str) else bytes(b)
    d = C.c_uint32()
    rc = L.zr_world_json_diff(ba, len(ba), bb, len(bb), C.byref(d))
    if rc:
        raise ZeldaRenderError(rc, "zr_world_json_diff: a payload does not parse")
    return d.value


def frame_delta_decode(tiles, offsets, stream, client):
    """zr_frame_delta_decode, the client's side of a packed delivery (host code only): tiles uint32[n], offsets uint32[n + 1], stream
    uint8[>= offsets[n]] applied in place to client, an (H, W, 4) uint8 copy of the frame.  A malformed delivery raises
    ZeldaRenderError(ZR_ERR_PARSE) and writes nothing."""
    tiles, offsets = np.ascontiguousarray(tiles, dtype=np.uint32), np.ascontiguousarray(offsets, dtype=np.uint32)
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    assert client.dtype == np.uint8 and client.ndim == 3 and client.shape[2] == 4 and client.flags.c_contiguous and client.flags.writeable
    assert offsets.size == tiles.size + 1
    rc = lib().zr_frame_delta_decode(_ptr(tiles), _ptr(offsets), tiles.size, _ptr(stream), stream.size, client.shape[1], client.shape[0], _ptr(client))
    if rc:
        raise ZeldaRenderError(rc, "zr_frame_delta_decode: the delivery is malformed")
    return client


def frame_scaled_extent(w, h, s):
    """zr_frame_scaled_extent: (ceil(w / s), ceil(h / s)) for s in 1..8"""
    wd, hd = C.c_uint32(), C.c_uint32()
    rc = lib().zr_frame_scaled_extent(w, h, s, C.byref(wd), C.byref(hd))
    if rc:
        raise ZeldaRenderError(rc, "zr_frame_scaled_extent: bad argument")
    return wd.value, hd.value


def frame_downscale(img, s):
    """zr_frame_downscale, the host statement of the scaled forms' filter (host code only): img (H, W, 4) uint8 box-filtered by s in
    linear light -> (ceil(H / s), ceil(W / s), 4) uint8"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    assert img.ndim == 3 and img.shape[2] == 4
    h, w = img.shape[:2]
    wd, hd = frame_scaled_extent(w, h, s)
    out = np.zeros((hd, wd, 4), dtype=np.uint8)
    rc = lib().zr_frame_downscale(_ptr(img), w, h, s, _ptr(out), out.nbytes)
    if rc:
        raise ZeldaRenderError(rc, "zr_frame_downscale: bad argument")
    return out


def _style(style):
    """an abi.HighlightStyle from one, from None (the default) or from a dict of make_highlight_style's arguments"""
    if isinstance(style, abi.HighlightStyle):
        return style
    return abi.make_highlight_style(**(style or {}))


def frame_highlight(img, mask, style=None):
    """zr_frame_highlight, the host statement of the highlight rule (host code only): img (H, W, 4) uint8, mask (H, W) non-zero where
    highlighted, style an abi.HighlightStyle (None: the default) -> (H, W, 4) uint8"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    assert img.ndim == 3 and img.shape[2] == 4 and mask.shape == img.shape[:2]
    st = _style(style)
    out = np.zeros_like(img)
    rc = lib().zr_frame_highlight(_ptr(img), _ptr(mask), img.shape[1], img.shape[0], C.byref(st), C.sizeof(st), _ptr(out), out.nbytes)
    if rc:
        raise ZeldaRenderError(rc, "zr_frame_highlight: bad argument")
    return out


def _overlay_style(style):
    """an abi.OverlayStyle from one, from None (the default) or from a dict of make_overlay_style's arguments"""
    if isinstance(style, abi.OverlayStyle):
        return style
    return abi.make_overlay_style(**(style or {}))


def frame_overlay(img, depth, pvm, segments, style=None):
    """zr_frame_overlay, the host statement of the overlay rule (host code only): img (H, W, 4) uint8, depth (H, W) float32, pvm the
    frame's proj * view * model (16 floats, column-major), segments an abi.OVERLAY_SEGMENT array (or make_overlay_segments' rows),
    style an abi.OverlayStyle (None: the default) -> (H, W, 4) uint8"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    pvm = np.ascontiguousarray(np.asarray(pvm, dtype=np.float32).reshape(16))
    seg = abi.make_overlay_segments(segments)
    assert img.ndim == 3 and img.shape[2] == 4 and depth.shape == img.shape[:2]
    st = _overlay_style(style)
    out = np.zeros_like(img)
    rc = lib().zr_frame_overlay(_ptr(img), _ptr(depth), img.shape[1], img.shape[0], _ptr(pvm), _ptr(seg) if seg.size else None, seg.size, C.byref(st), C.sizeof(st),
                                _ptr(out), out.nbytes)
    if rc:
        raise ZeldaRenderError(rc, "zr_frame_overlay: bad argument")
    return out


def _wire_style(style):
    """an abi.WireStyle from one, from None (the default) or from a dict of make_wire_style's arguments"""
    if isinstance(style, abi.WireStyle):
        return style
    return abi.make_wire_style(**(style or {}))


def frame_wire(img, prim, corners, style=None, selected=None):
    """zr_frame_wire, the host statement of the wireframe rule (host code only): img (H, W, 4) uint8, prim (H, W) uint32 winners
    (read_ids(IDS_PRIMITIVE)), corners (n, 3, 3) float32 - x, y, w of each primitive's three clip-space corners - style an abi.WireStyle
    (None: the default), selected n flags (read only with WIRE_SELECTED) or None: every primitive -> (H, W, 4) uint8"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    prim = np.ascontiguousarray(prim, dtype=np.uint32)
    corners = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 9)
    assert img.ndim == 3 and img.shape[2] == 4 and prim.shape == img.shape[:2]
    if selected is not None:
        selected = np.ascontiguousarray(np.asarray(selected) != 0, dtype=np.uint8).reshape(-1)
        assert selected.size == len(corners)
    st = _wire_style(style)
    out = np.zeros_like(img)
    rc = lib().zr_frame_wire(_ptr(img), _ptr(prim), img.shape[1], img.shape[0], _ptr(corners) if len(corners) else None, len(corners),
                             _ptr(selected) if selected is not None and selected.size else None, C.byref(st), C.sizeof(st), _ptr(out), out.nbytes)
    if rc:
        raise ZeldaRenderError(rc, "zr_frame_wire: bad argument")
    return out


def _rays(rays):
    rays = np.ascontiguousarray(rays)
    if rays.dtype != abi.RAY:
        raise TypeError("rays: an abi.RAY array (abi.make_rays)")
    return rays.reshape(-1)


def ray_triangles(rays, tris, flags=0):
    """The ray / triangle rule on the host, context-free (zr_ray_triangles): abi.RAY rays against (n, 3, 3) float32 world triangles ->
    abi.RAY_RECORD records; a hit's triangle is the index into tris, its object and instance 0."""
    rays = _rays(rays)
    tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    hits = np.zeros(len(rays), dtype=abi.RAY_RECORD)
    rc = lib().zr_ray_triangles(_ptr(rays), len(rays), _ptr(tris), len(tris), flags, _ptr(hits))
    if rc != 0:
        raise ZeldaRenderError(rc, "zr_ray_triangles: bad argument")
    return hits


def _delta_dict(d):
    return {k: getattr(d, k) for k, _ in abi.WorldDelta._fields_ if k not in ("struct_bytes", "reserved")}


class Renderer:
    def __init__(self, width=1920, height=1080, shadow_dim=1024, device=0, tile_rank=0, tile_world=1, flags=0,
                 debug_view=0):
        self.L = lib()
        self.W, self.H, self.SD = width, height, shadow_dim
        self.tile_rank, self.tile_world = tile_rank, tile_world
        cfg = abi.Config(width, height, shadow_dim, debug_view, device, tile_rank, tile_world, flags)
        h = C.c_void_p()
        rc = self.L.zr_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise ZeldaRenderError(rc, "zr_create failed (no usable HIP device or bad config); there is no CPU fallback")
        self.h = h

    # ---- plumbing
    def _chk(self, rc):
        if rc != 0:
            raise ZeldaRenderError(rc, (self.L.zr_last_error(self.h) or b"").decode(errors="replace"))

    def close(self):
        if getattr(self, "h", None):
            self.L.zr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def resize(self, width, height):
        """zr_resize: a new extent, the same scene - nothing is submitted again, and every later frame is a new context's at that extent.
        Device pointers the context handed out (color_device_ptr, tiles_device_buffer) are void afterwards."""
        self._chk(self.L.zr_resize(self.h, width, height))
        self.W, self.H = self.extent()

    def extent(self):
        """zr_get_extent: (width, height) as the context has them now"""
        w, h = C.c_uint32(), C.c_uint32()
        self._chk(self.L.zr_get_extent(self.h, C.byref(w), C.byref(h)))
        return w.value, h.value

    def set_stream(self, hip_stream):
        self._chk(self.L.zr_set_stream(self.h, C.c_void_p(hip_stream)))

    # ---- scene
    def mesh_create(self, verts, idx):
        verts = np.ascontiguousarray(verts)
        assert verts.dtype == abi.XkVertex
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        mid = C.c_uint32()
        self._chk(self.L.zr_mesh_create(self.h, _ptr(verts), len(verts), _ptr(idx), len(idx), C.byref(mid)))
        return mid.value

    def mesh_set_meshlets(self, mesh, meshlets, mverts, mtris):
        meshlets = np.ascontiguousarray(meshlets)
        assert meshlets.dtype == abi.XkMeshlet
        mverts = np.ascontiguousarray(mverts, dtype=np.uint32)
        mtris = np.ascontiguousarray(mtris, dtype=np.uint8)
        self._chk(self.L.zr_mesh_set_meshlets(self.h, mesh, _ptr(meshlets), len(meshlets), _ptr(mverts), len(mverts),
                                              _ptr(mtris), len(mtris)))

    def mesh_build_meshlets(self, mesh, max_vertices=64, max_triangles=124, cone_weight=0.2):
        self._chk(self.L.zr_mesh_build_meshlets(self.h, mesh, max_vertices, max_triangles, cone_weight))

    def mesh_get_meshlets(self, mesh):
        nm, nmv, nmt = C.c_uint32(), C.c_size_t(), C.c_size_t()
        self._chk(self.L.zr_mesh_get_meshlets(self.h, mesh, None, C.byref(nm), None, C.byref(nmv), None, C.byref(nmt)))
        ml = np.zeros(nm.value, dtype=abi.XkMeshlet)
        mv = np.zeros(nmv.value, dtype=np.uint32)
        mt = np.zeros(nmt.value, dtype=np.uint8)
        self._chk(self.L.zr_mesh_get_meshlets(self.h, mesh, _ptr(ml), C.byref(nm), _ptr(mv), C.byref(nmv), _ptr(mt),
                                              C.byref(nmt)))
        return ml, mv, mt

    def object_add(self, mesh, material=None, instances=None):
        mat = C.cast(C.pointer(material), C.c_void_p) if material is not None else None
        n = 0 if instances is None else len(instances)
        inst = np.ascontiguousarray(instances) if n else None
        if n:
            assert inst.dtype == abi.XkInstanceData
        self._chk(self.L.zr_object_add(self.h, mesh, mat, _ptr(inst) if n else None, n))

    def scene_clear(self):
        self._chk(self.L.zr_scene_clear(self.h))

    def set_limits(self, record_chunks=0, slow_triangles=0):
        """Capacities of the triangle-record arrays (chunks of 256 records, `zr_record_chunk_size()`) and the clipped-triangle list; 0 = defaults."""
        self._chk(self.L.zr_set_limits(self.h, record_chunks, slow_triangles))

    def set_bucket_share(self, percent=100):
        """Plan every per-tile record bucket at `percent` of its size (zr_set_bucket_share): the rest goes the overflow route - same frame."""
        self._chk(self.L.zr_set_bucket_share(self.h, percent))

    def object_count(self):
        n = C.c_uint32()
        self._chk(self.L.zr_object_count(self.h, C.byref(n)))
        return n.value

    def object_get_instances(self, index):
        n, mesh = C.c_uint32(), C.c_uint32()
        self._chk(self.L.zr_object_get_instances(self.h, index, C.byref(mesh), None, C.byref(n)))
        inst = np.zeros(n.value, dtype=abi.XkInstanceData)
        if n.value:
            self._chk(self.L.zr_object_get_instances(self.h, index, C.byref(mesh), _ptr(inst), C.byref(n)))
        return mesh.value, (inst if n.value else None)

    def object_set_instances(self, index, instances, first=0):
        """Replace instances [first, first + len(instances)) of instanced object `index` (an abi.XkInstanceData array) from the next
        frame on (zr_object_set_instances); frames already enqueued keep the old values."""
        inst = np.ascontiguousarray(instances)
        assert inst.dtype == abi.XkInstanceData
        self._chk(self.L.zr_object_set_instances(self.h, index, first, _ptr(inst), inst.size))

    def object_update_instances_async(self, index, data, idx=None, first=0, stream=None):
        """The same from device tensors, in the order of `stream` (a torch.cuda.Stream or a HIP stream handle; None = the render stream):
        data = uint8 [n, 32] (or any contiguous view of n XkInstanceData), idx = None (instances first .. first + n - 1) or int32 [n]
        (the object's own indices; those >= its instance count are ignored).  Both may be overwritten by work enqueued on `stream`
        afterwards (zr_object_update_instances_async)."""
        assert data.is_cuda and data.is_contiguous() and data.numel() * data.element_size() % abi.XkInstanceData.itemsize == 0
        n = data.numel() * data.element_size() // abi.XkInstanceData.itemsize
        if idx is not None:
            assert idx.is_cuda and idx.is_contiguous() and idx.element_size() == 4 and idx.numel() == n
        h = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        self._chk(self.L.zr_object_update_instances_async(self.h, index, first, C.c_void_p(idx.data_ptr()) if idx is not None else None,
                                                          C.c_void_p(data.data_ptr()) if n else None, n, C.c_void_p(h) if h else None))

    def object_set_visible(self, index, visible=True):
        """Show or hide object `index` as a whole (instanced or not) from the next frame on (zr_object_set_visible); its instances'
        own bytes stay as they are."""
        self._chk(self.L.zr_object_set_visible(self.h, index, 1 if visible else 0))

    def object_set_instance_visibility(self, index, visible, first=0):
        """Show (nonzero) or hide (0) instances [first, first + len(visible)) of instanced object `index` from the next frame on
        (zr_object_set_instance_visibility); frames already enqueued keep the old state."""
        vis = np.ascontiguousarray(np.asarray(visible) != 0, dtype=np.uint8)
        self._chk(self.L.zr_object_set_instance_visibility(self.h, index, first, _ptr(vis), vis.size))

    def object_update_instance_visibility_async(self, index, visible, idx=None, first=0, stream=None, n=None):
        """The same from device memory, in the order of `stream` (a torch.cuda.Stream or a HIP stream handle; None = the render stream):
        visible = a contiguous CUDA tensor of n one-byte elements (uint8 or bool), idx = None (instances first .. first + n - 1) or
        int32 [n] (the object's own indices; those >= its instance count are ignored) - or raw device pointers with `n`.  Both may be
        overwritten by work enqueued on `stream` afterwards (zr_object_update_instance_visibility_async)."""
        if hasattr(visible, "data_ptr"):
            assert visible.is_cuda and visible.is_contiguous() and visible.element_size() == 1
            n = visible.numel()
            vptr = visible.data_ptr() if n else 0
        else:
            assert n is not None, "a raw device pointer needs n, the number of instances"
            vptr = int(visible) if visible else 0
        if idx is not None and hasattr(idx, "data_ptr"):
            assert idx.is_cuda and idx.is_contiguous() and idx.element_size() == 4 and idx.numel() == n
            iptr = idx.data_ptr()
        else:
            iptr = int(idx) if idx else 0
        h = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        self._chk(self.L.zr_object_update_instance_visibility_async(self.h, index, first, C.c_void_p(iptr) if iptr else None,
                                                                    C.c_void_p(vptr) if vptr else None, n, C.c_void_p(h) if h else None))

    def object_get_visibility(self, index):
        """(object visible, uint8 array of one byte per instance - None for a non-instanced draw) (zr_object_get_visibility)."""
        n, ov = C.c_uint32(), C.c_int()
        self._chk(self.L.zr_object_get_visibility(self.h, index, C.byref(ov), None, C.byref(n)))
        vis = np.zeros(n.value, dtype=np.uint8)
        if n.value:
            self._chk(self.L.zr_object_get_visibility(self.h, index, C.byref(ov), _ptr(vis), C.byref(n)))
        return bool(ov.value), (vis if n.value else None)

    def mesh_set_vertices(self, mesh, verts, first=0):
        """Replace vertices [first, first + len(verts)) of `mesh` (an abi.XkVertex array) from the next frame on (zr_mesh_set_vertices);
        frames already enqueued keep the old shape.  Counts, indices and the meshlet partition stay; the bounds are refitted."""
        verts = np.ascontiguousarray(verts)
        assert verts.dtype == abi.XkVertex
        self._chk(self.L.zr_mesh_set_vertices(self.h, mesh, first, _ptr(verts), verts.size))

    def mesh_update_vertices_async(self, mesh, data, first=0, stream=None, n=None):
        """The same from device memory, in the order of `stream` (a torch.cuda.Stream or a HIP stream handle; None = the render stream):
        data = a contiguous CUDA tensor holding whole XkVertex records (e.g. float32 [n, 11]), or a device pointer with `n` vertices.
        It may be overwritten by work enqueued on `stream` afterwards (zr_mesh_update_vertices_async)."""
        if hasattr(data, "data_ptr"):
            assert data.is_cuda and data.is_contiguous() and data.numel() * data.element_size() % abi.XkVertex.itemsize == 0
            n = data.numel() * data.element_size() // abi.XkVertex.itemsize
            ptr = data.data_ptr()
        else:
            assert n is not None, "a raw device pointer needs n, the number of vertices"
            ptr = int(data) if data else 0
        h = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        self._chk(self.L.zr_mesh_update_vertices_async(self.h, mesh, first, C.c_void_p(ptr) if ptr else None, n, C.c_void_p(h) if h else None))

    def mesh_get_vertices(self, mesh):
        n = C.c_uint32()
        self._chk(self.L.zr_mesh_get_vertices(self.h, mesh, None, C.byref(n)))
        verts = np.zeros(n.value, dtype=abi.XkVertex)
        self._chk(self.L.zr_mesh_get_vertices(self.h, mesh, _ptr(verts), C.byref(n)))
        return verts

    def object_set_texture(self, index, slot, image):
        """Replace the image of material slot `slot` (0..6, abi.TEXTURE_SLOTS) of object `index` with a uint8 [h, w, 4] array of the
        slot's own size, from the next frame on (zr_object_set_texture); frames already enqueued keep the old image.  Every mip level and
        the packed material follow on the GPU."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        assert img.ndim == 3 and img.shape[2] == 4
        im = abi.Image(img.ctypes.data, img.shape[1], img.shape[0])
        self._chk(self.L.zr_object_set_texture(self.h, index, slot, C.byref(im)))

    def object_update_texture_async(self, index, slot, data, stream=None):
        """The same from a contiguous CUDA uint8 tensor [h, w, 4], in the order of `stream` (a torch.cuda.Stream or a HIP stream handle;
        None = the render stream).  It may be overwritten by work enqueued on `stream` afterwards (zr_object_update_texture_async)."""
        assert data.is_cuda and data.is_contiguous() and data.element_size() == 1 and data.dim() == 3 and data.shape[2] == 4
        h = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        self._chk(self.L.zr_object_update_texture_async(self.h, index, slot, C.c_void_p(data.data_ptr()), data.shape[1], data.shape[0],
                                                        C.c_void_p(h) if h else None))

    def object_get_texture(self, index, slot):
        """The slot's current mip chain: a list of uint8 [h, w, 4] arrays, level 0 first (zr_object_get_texture)."""
        w, h, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.L.zr_object_get_texture(self.h, index, slot, 0, None, 0, C.byref(w), C.byref(h), C.byref(n)))
        out = []
        for level in range(n.value):
            self._chk(self.L.zr_object_get_texture(self.h, index, slot, level, None, 0, C.byref(w), C.byref(h), C.byref(n)))
            a = np.zeros((h.value, w.value, 4), dtype=np.uint8)
            self._chk(self.L.zr_object_get_texture(self.h, index, slot, level, _ptr(a), a.nbytes, C.byref(w), C.byref(h), C.byref(n)))
            out.append(a)
        return out

    def set_cubemap(self, faces):
        if faces is None:
            self._chk(self.L.zr_set_cubemap(self.h, None, 0))
            return
        faces = [np.ascontiguousarray(f, dtype=np.uint8) for f in faces]
        assert len(faces) == 6 and all(f.shape == faces[0].shape and f.shape[0] == f.shape[1] and f.shape[2] == 4 for f in faces)
        arr = (C.c_void_p * 6)(*[f.ctypes.data for f in faces])
        self._chk(self.L.zr_set_cubemap(self.h, arr, faces[0].shape[0]))

    def set_skydome(self, verts, idx, image):
        """Sky mesh + its sRGB RGBA8 image (H, W, 4); image None removes the pass (CreateSkydomePass, ZE:2690-2744)."""
        if image is None:
            self._chk(self.L.zr_set_skydome(self.h, None, 0, None, 0, None))
            return
        verts = np.ascontiguousarray(verts)
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        img = np.ascontiguousarray(image, dtype=np.uint8)
        im = abi.Image(img.ctypes.data, img.shape[1], img.shape[0])
        self._chk(self.L.zr_set_skydome(self.h, _ptr(verts), len(verts), _ptr(idx), len(idx), C.cast(C.pointer(im), C.c_void_p)))

    def set_background(self, image):
        if image is None:
            self._chk(self.L.zr_set_background(self.h, None))
            return
        img = np.ascontiguousarray(image, dtype=np.uint8)
        im = abi.Image(img.ctypes.data, img.shape[1], img.shape[0])
        self._chk(self.L.zr_set_background(self.h, C.cast(C.pointer(im), C.c_void_p)))

    def set_sky_flags(self, enable_skydome=True, enable_background=True):
        self._chk(self.L.zr_set_sky_flags(self.h, int(enable_skydome), int(enable_background)))

    # ---- uniforms
    def update_uniforms(self, cam, dir_l, point_l, spot_l, roll_stage=0.0, roll_light=0.0, time=0.0):
        self._chk(self.L.zr_update_uniforms(self.h, *uniform_arguments(cam, dir_l, point_l, spot_l), roll_stage, roll_light, time))

    def set_frame(self, cam, shadow, view):
        self._chk(self.L.zr_set_frame(self.h, cam.ctypes.data, shadow.ctypes.data, view.ctypes.data))

    def get_frame(self):
        cam = np.zeros((), dtype=abi.XkUniformBufferMVP)
        sh = np.zeros((), dtype=abi.XkUniformBufferMVP)
        view = np.zeros((), dtype=abi.XkView)
        self._chk(self.L.zr_get_frame(self.h, cam.ctypes.data, sh.ctypes.data, view.ctypes.data))
        return cam, sh, view

    def set_debug_view(self, v):
        self._chk(self.L.zr_set_debug_view(self.h, v))

    def set_shading(self, forward):
        """False: the deferred frame (default); True: the forward variant, SH/Base.frag (zr_set_shading)."""
        self._chk(self.L.zr_set_shading(self.h, 1 if forward else 0))

    # ---- frame
    def render(self, debug_view=None, passes=None):
        if debug_view is not None:
            self.set_debug_view(debug_view)
        self._chk(self.L.zr_render(self.h))

    def render_shadow(self):
        self._chk(self.L.zr_render_shadow(self.h))

    def render_gbuffer(self):
        self._chk(self.L.zr_render_gbuffer(self.h))

    def render_lighting(self):
        self._chk(self.L.zr_render_lighting(self.h))

    def render_geometry(self):
        """Shadow pass and deferred-scene pass side by side (not joined: see stream_wait_shadow)."""
        self._chk(self.L.zr_render_geometry(self.h))

    def stream_wait_shadow(self, hip_stream):
        """Make a HIP stream (its raw handle) wait for the shadow pass enqueued last."""
        self._chk(self.L.zr_stream_wait_shadow(self.h, hip_stream))

    def set_shadow_partition(self, rank, world):
        self._chk(self.L.zr_set_shadow_partition(self.h, rank, world))

    def set_shadow_tiles(self, rank, world):
        """The shadow MAP owned by light-space super-tiles: this context draws the casters that reach its tiles (exact there)."""
        self._chk(self.L.zr_set_shadow_tiles(self.h, rank, world))

    def shadow_tiles_bytes(self):
        n = C.c_size_t()
        self._chk(self.L.zr_shadow_tiles_bytes(self.h, C.byref(n)))
        return n.value

    def shadow_pack(self, packed_dev, hip_stream=None):
        self._chk(self.L.zr_shadow_pack(self.h, C.c_void_p(packed_dev), C.c_void_p(hip_stream) if hip_stream else None))

    def shadow_unpack(self, gathered_dev, hip_stream=None):
        self._chk(self.L.zr_shadow_unpack(self.h, C.c_void_p(gathered_dev), C.c_void_p(hip_stream) if hip_stream else None))

    def set_shadow_buffer(self, dev_ptr):
        self._chk(self.L.zr_set_shadow_buffer(self.h, C.c_void_p(dev_ptr) if dev_ptr else None))

    def finish(self):
        self._chk(self.L.zr_finish(self.h))

    def set_timing_interval(self, interval):
        """Record the per-pass hipEvents on every interval-th frame only (each record is a ~6 us bubble on the stream)."""
        self._chk(self.L.zr_set_timing_interval(self.h, interval))

    def pass_times(self, last_n=1):
        """Mean GPU milliseconds per pass over the last `last_n` (<= 64) timed frames."""
        ms = (C.c_float * len(abi.PASS_NAMES))()
        self._chk(self.L.zr_get_pass_times_avg(self.h, last_n, ms))
        return dict(zip(abi.PASS_NAMES, [float(x) for x in ms]))

    def frame_latencies(self, n=64):
        """Begin-to-end GPU milliseconds of the last n (<= 64) timed frames, newest first."""
        ms = (C.c_float * n)()
        got = self.L.zr_get_frame_latencies(self.h, n, ms)
        if got < 0:
            self._chk(got)
        return [float(ms[i]) for i in range(got)]

    def frame_periods(self, n=511):
        """GPU milliseconds between the ends of consecutive frames for the last n (<= 511) frames, newest first."""
        ms = (C.c_float * n)()
        got = self.L.zr_get_frame_periods(self.h, n, ms)
        if got < 0:
            self._chk(got)
        return [float(ms[i]) for i in range(got)]

    def stats(self):
        s = abi.Stats()
        self._chk(self.L.zr_get_stats(self.h, C.byref(s), C.sizeof(s)))
        return {"work_items": list(s.work_items), "survivors": list(s.survivors), "bin_entries": list(s.bin_entries),
                "covered_pixels": int(s.covered_pixels), "covered_shadow_texels": int(s.covered_shadow_texels), "overflow": int(s.overflow),
                "hiz_culled": int(s.hiz_culled), "hiz_culled_geom": int(s.hiz_culled_geom), "round1_survivors": int(s.round1_survivors),
                "shadow_occluded": int(s.shadow_occluded), "shadow_late": int(s.shadow_late)}

    def light_keep(self):
        """What the last frame's lighting pass did with the plane of standing terms ("ignored" / "filled" / "read": zr_get_light_keep), and
        how many frames did each so far."""
        k = abi.LightKeep()
        self._chk(self.L.zr_get_light_keep(self.h, C.byref(k), C.sizeof(k)))
        return {"last": ("ignored", "filled", "read")[int(k.last)], "ignored": int(k.ignored), "filled": int(k.filled), "read": int(k.read),
                "plane_bytes": int(k.plane_bytes), "read_by_arg": int(k.read_by_arg)}

    def rest_settled(self):
        """(parts, settled) of the resting frame's one launch (zr_get_rest_settled): how many of its half-tile parts stand settled after
        the frame enqueued last - no point light reaches them and their pixels are left as they are.  Waits for the frame."""
        parts, settled = C.c_uint32(), C.c_uint32()
        self._chk(self.L.zr_get_rest_settled(self.h, C.byref(parts), C.byref(settled)))
        return int(parts.value), int(settled.value)

    def rest_settled_parts(self):
        """zr_get_rest_settled_parts: a uint8 per part of the resting frame's launch (owned tile slot * 2 + half), 1 where it stands settled"""
        out = np.zeros(self.rest_settled()[0], dtype=np.uint8)
        self._chk(self.L.zr_get_rest_settled_parts(self.h, _ptr(out) if out.size else None, out.nbytes))
        return out

    # ---- read-back
    def color(self):
        out = np.zeros((self.H, self.W, 4), dtype=np.uint8)
        self._chk(self.L.zr_read_color(self.h, _ptr(out), out.nbytes))
        return out

    def gbuffer(self, target):
        out = np.zeros((self.H, self.W), dtype=abi.GBUFFER_DTYPES[target])
        self._chk(self.L.zr_read_gbuffer(self.h, target, _ptr(out), out.nbytes))
        return out

    def shadowmap(self):
        out = np.zeros((self.SD, self.SD), dtype=np.float32)
        self._chk(self.L.zr_read_shadowmap(self.h, _ptr(out), out.nbytes))
        return out

    def copy_frame_async(self, color_dev=None, shadow_dev=None):
        """The frame enqueued last -> caller-owned device buffers (addresses), in stream order, no host synchronisation."""
        self._chk(self.L.zr_copy_frame_async(self.h, C.c_void_p(color_dev) if color_dev else None, C.c_void_p(shadow_dev) if shadow_dev else None))

    # ---- delivering changes: the frame as the tiles that differ from what was delivered last
    def set_frame_delta(self, on=True):
        """Keep a delivered copy of the frame and deliver differences against it (default off; allocates on enable).
        on = abi.FRAME_DELTA_PACKED enables the packed forms as well."""
        self._chk(self.L.zr_set_frame_delta(self.h, int(on)))

    def frame_delta_reset(self):
        """A new client: the next delivery lists every tile again."""
        self._chk(self.L.zr_frame_delta_reset(self.h))

    def frame_delta_tiles(self):
        """How many 32 x 32 tiles the delivered frame has - the frame, at a delta scale above 1 the scaled one: the size every delivery's
        buffers are made for."""
        return self.frame_delta_extent()[2]

    def set_frame_delta_scale(self, s):
        """The scale the deliveries of changes work at (default 1; only while delta is off, kept across set_frame_delta(False))."""
        self._chk(self.L.zr_set_frame_delta_scale(self.h, s))

    def frame_delta_extent(self):
        """zr_get_frame_delta_extent: (width, height, total_tiles, scale) of what the deliveries of changes deliver."""
        w, h, t, s = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.L.zr_get_frame_delta_extent(self.h, C.byref(w), C.byref(h), C.byref(t), C.byref(s)))
        return w.value, h.value, t.value, s.value

    # ---- delivering a scaled frame: box-filtered by an integer factor in linear light, on the GPU
    def _scaled_shape(self, s):
        """(ceil(H / s), ceil(W / s), 4); s = 0 gets a shape too, so that it reaches the library and comes back as ZR_ERR_ARG"""
        s = max(s, 1)
        return -(-self.H // s), -(-self.W // s), 4

    def color_scaled(self, s):
        """zr_read_color_scaled: the frame filtered by s (1..8) -> (ceil(H / s), ceil(W / s), 4) uint8"""
        out = np.zeros(self._scaled_shape(s), dtype=np.uint8)
        self._chk(self.L.zr_read_color_scaled(self.h, s, _ptr(out), out.nbytes))
        return out

    def copy_frame_scaled_async(self, s, color_dev):
        """The frame enqueued last filtered by s -> a caller-owned device buffer (address, 4-byte aligned, ceil(W / s) * ceil(H / s) * 4
        bytes), in stream order, no host synchronisation."""
        self._chk(self.L.zr_copy_frame_scaled_async(self.h, s, C.c_void_p(color_dev) if color_dev else None))

    # ---- highlighting a selection: an outline round, and a fill over, a set of instances in the delivered frame
    def highlight_set(self, obj, on=True, first=0):
        """zr_highlight_set: instances first .. of object `obj` into (non-zero) or out of (0) the set; on: a flag per instance, or one
        flag for a non-instanced object / the single instance `first`"""
        on = np.ascontiguousarray(np.atleast_1d(np.asarray(on)) != 0, dtype=np.uint8)
        self._chk(self.L.zr_highlight_set(self.h, obj, first, _ptr(on), on.size))

    def highlight_clear(self):
        self._chk(self.L.zr_highlight_clear(self.h))

    def highlight_get(self):
        """The set, a byte per slot of instance_coverage"""
        out = np.zeros(self.instance_slots()[1], dtype=np.uint8)
        self._chk(self.L.zr_highlight_get(self.h, _ptr(out) if out.size else None, out.nbytes))
        return out

    def set_highlight_style(self, style=None, **kw):
        """zr_set_highlight_style: an abi.HighlightStyle, or make_highlight_style's arguments (outline=, fill=, radius=)"""
        st = _style(style if style is not None else kw)
        self._chk(self.L.zr_set_highlight_style(self.h, C.byref(st), C.sizeof(st)))

    def highlight_style(self):
        st = abi.HighlightStyle()
        self._chk(self.L.zr_get_highlight_style(self.h, C.byref(st), C.sizeof(st)))
        return st

    def color_highlighted(self, s=1):
        """zr_read_color_highlighted: the frame with the set outlined and filled, filtered by s (1..8) -> (ceil(H / s), ceil(W / s), 4) uint8"""
        out = np.zeros(self._scaled_shape(s), dtype=np.uint8)
        self._chk(self.L.zr_read_color_highlighted(self.h, s, _ptr(out), out.nbytes))
        return out

    def copy_frame_highlighted_async(self, s, color_dev):
        """The frame enqueued last, highlighted and filtered by s -> a caller-owned device buffer (address, 4-byte aligned, ceil(W / s) *
        ceil(H / s) * 4 bytes), in stream order, no host synchronisation."""
        self._chk(self.L.zr_copy_frame_highlighted_async(self.h, s, C.c_void_p(color_dev) if color_dev else None))

    # ---- overlaying lines: depth-tested segments drawn over the delivered frame
    def overlay_set(self, segments=None):
        """zr_overlay_set: replaces the list; an abi.OVERLAY_SEGMENT array, rows (ax, ay, az, bx, by, bz, r, g, b, a[, flags]), or
        None / empty: cleared"""
        seg = abi.make_overlay_segments(segments if segments is not None else [])
        self._chk(self.L.zr_overlay_set(self.h, _ptr(seg) if seg.size else None, seg.size))

    def overlay_get(self):
        """zr_overlay_get -> an abi.OVERLAY_SEGMENT array"""
        n = C.c_uint32(0)
        self._chk(self.L.zr_overlay_get(self.h, None, C.byref(n)))
        out = np.zeros(n.value, dtype=abi.OVERLAY_SEGMENT)
        self._chk(self.L.zr_overlay_get(self.h, _ptr(out) if out.size else None, C.byref(n)))
        return out

    def overlay_style(self, style=None, **kw):
        """zr_get_overlay_style with no argument -> abi.OverlayStyle; with an abi.OverlayStyle or make_overlay_style's arguments
        (depth_bias=, hidden_opacity=): zr_set_overlay_style"""
        if style is None and not kw:
            st = abi.OverlayStyle()
            self._chk(self.L.zr_get_overlay_style(self.h, C.byref(st), C.sizeof(st)))
            return st
        st = _overlay_style(style if style is not None else kw)
        self._chk(self.L.zr_set_overlay_style(self.h, C.byref(st), C.sizeof(st)))
        return st

    def read_color_overlaid(self, s=1, highlight=False):
        """zr_read_color_overlaid: the frame (highlighted underneath or not) with the list's lines over it, filtered by s (1..8) ->
        (ceil(H / s), ceil(W / s), 4) uint8"""
        out = np.zeros(self._scaled_shape(s), dtype=np.uint8)
        self._chk(self.L.zr_read_color_overlaid(self.h, s, 1 if highlight else 0, _ptr(out), out.nbytes))
        return out

    def copy_frame_overlaid_async(self, s, highlight, color_dev):
        """The frame enqueued last, overlaid and filtered by s -> a caller-owned device buffer (address, 4-byte aligned, ceil(W / s) *
        ceil(H / s) * 4 bytes), in stream order, no host synchronisation."""
        self._chk(self.L.zr_copy_frame_overlaid_async(self.h, s, 1 if highlight else 0, C.c_void_p(color_dev) if color_dev else None))

    # ---- the wireframe: the visible triangles' edges drawn over the delivered frame
    def set_wire_style(self, style=None, **kw):
        """zr_set_wire_style: an abi.WireStyle, or make_wire_style's arguments (rgba=, width_256=, flags=)"""
        st = _wire_style(style if style is not None else kw)
        self._chk(self.L.zr_set_wire_style(self.h, C.byref(st), C.sizeof(st)))

    def wire_style(self):
        st = abi.WireStyle()
        self._chk(self.L.zr_get_wire_style(self.h, C.byref(st), C.sizeof(st)))
        return st

    def read_color_staged(self, stages, s=1):
        """zr_read_color_staged: the frame with the stages of the mask (abi.STAGE_WIRE | STAGE_HIGHLIGHT | STAGE_OVERLAY) applied in that
        order, filtered by s (1..8) -> (ceil(H / s), ceil(W / s), 4) uint8"""
        out = np.zeros(self._scaled_shape(s), dtype=np.uint8)
        self._chk(self.L.zr_read_color_staged(self.h, stages, s, _ptr(out), out.nbytes))
        return out

    def copy_frame_staged_async(self, stages, s, color_dev):
        """The frame enqueued last with the stages of the mask applied, filtered by s -> a caller-owned device buffer (address, 4-byte
        aligned, ceil(W / s) * ceil(H / s) * 4 bytes), in stream order, no host synchronisation."""
        self._chk(self.L.zr_copy_frame_staged_async(self.h, stages, s, C.c_void_p(color_dev) if color_dev else None))

    def set_frame_delta_wire(self, on=True):
        """The deliveries of changes carry the wire (default off; only while delta is off, kept across set_frame_delta(False))."""
        self._chk(self.L.zr_set_frame_delta_wire(self.h, 1 if on else 0))

    def set_frame_delta_overlay(self, on=True):
        """The deliveries of changes deliver the overlaid frame (default off; only while delta is off, kept across set_frame_delta(False))."""
        self._chk(self.L.zr_set_frame_delta_overlay(self.h, 1 if on else 0))

    def set_frame_delta_highlight(self, on=True):
        """The deliveries of changes deliver the highlighted frame (default off; only while delta is off, kept across set_frame_delta(False))."""
        self._chk(self.L.zr_set_frame_delta_highlight(self.h, 1 if on else 0))

    def read_frame_delta(self, tiles=None, pixels=None):
        """One delivery to the host: (tiles[n] uint32 ascending, pixels[n, 32, 32, 4] uint8, header dict).  tiles / pixels: full-sized
        buffers to deliver into (uint32[total], uint8[total, 32, 32, 4]); only their first n entries are written."""
        total = self.frame_delta_tiles()
        if tiles is None:
            tiles = np.zeros(total, dtype=np.uint32)
        if pixels is None:
            pixels = np.zeros((total, abi.TILE, abi.TILE, 4), dtype=np.uint8)
        assert tiles.dtype == np.uint32 and pixels.dtype == np.uint8 and tiles.flags.c_contiguous and pixels.flags.c_contiguous
        h = abi.FrameDelta()
        self._chk(self.L.zr_read_frame_delta(self.h, _ptr(tiles), tiles.size, _ptr(pixels), pixels.nbytes, C.byref(h), C.sizeof(h)))
        header = {k: int(getattr(h, k)) for k, _ in abi.FrameDelta._fields_}
        return tiles[:h.n_tiles], pixels.reshape(-1, abi.TILE, abi.TILE, 4)[:h.n_tiles], header

    def copy_frame_delta_async(self, header_dev, tiles_dev, pixels_dev):
        """One delivery into caller-owned device buffers (addresses: 16 bytes, total uint32, total * 4096 bytes), on the render stream,
        without a host sync."""
        self._chk(self.L.zr_copy_frame_delta_async(self.h, C.c_void_p(header_dev), C.c_void_p(tiles_dev), C.c_void_p(pixels_dev)))

    def read_frame_delta_packed(self, tiles=None, offsets=None, stream=None):
        """One packed delivery to the host: (tiles[n] uint32 ascending, offsets[n + 1] uint32, stream[bytes] uint8, header dict).  tiles /
        offsets / stream: full-sized buffers to deliver into (uint32[total], uint32[total + 1], uint8[total * abi.RECORD_MAX_BYTES]);
        only their first n, n + 1 and `bytes` entries are written."""
        total = self.frame_delta_tiles()
        tiles = np.zeros(total, dtype=np.uint32) if tiles is None else tiles
        offsets = np.zeros(total + 1, dtype=np.uint32) if offsets is None else offsets
        stream = np.zeros(total * abi.RECORD_MAX_BYTES, dtype=np.uint8) if stream is None else stream
        assert tiles.dtype == np.uint32 and offsets.dtype == np.uint32 and stream.dtype == np.uint8
        assert tiles.flags.c_contiguous and offsets.flags.c_contiguous and stream.flags.c_contiguous
        h = abi.FrameDeltaPacked()
        self._chk(self.L.zr_read_frame_delta_packed(self.h, _ptr(tiles), tiles.size, _ptr(offsets), offsets.size, _ptr(stream), stream.nbytes,
                                                    C.byref(h), C.sizeof(h)))
        header = {k: int(getattr(h, k)) for k, _ in abi.FrameDeltaPacked._fields_ if k != "reserved"}
        return tiles[:h.n_tiles], offsets[:h.n_tiles + 1], stream.reshape(-1)[:h.bytes], header

    def copy_frame_delta_packed_async(self, header_dev, tiles_dev, offsets_dev, stream_dev):
        """One packed delivery into caller-owned device buffers (addresses: 32 bytes, total uint32, total + 1 uint32, total *
        abi.RECORD_MAX_BYTES bytes 16-byte aligned), on the render stream, without a host sync."""
        self._chk(self.L.zr_copy_frame_delta_packed_async(self.h, C.c_void_p(header_dev), C.c_void_p(tiles_dev), C.c_void_p(offsets_dev),
                                                          C.c_void_p(stream_dev)))

    # ---- object identity of the last frame
    def set_id_capture(self, on=True):
        """Keep the deferred-scene pass's per-pixel winner from the next frame on (default off)."""
        self._chk(self.L.zr_set_id_capture(self.h, 1 if on else 0))

    def read_ids(self, kind=abi.IDS_PRIMITIVE):
        """IDS_PRIMITIVE: (H, W) uint32 primitive ids; IDS_OBJECT: (H, W, 2) uint32 {object, instance}; all ones = none."""
        out = np.zeros((self.H, self.W) if kind == abi.IDS_PRIMITIVE else (self.H, self.W, 2), dtype=np.uint32)
        self._chk(self.L.zr_read_ids(self.h, kind, _ptr(out), out.nbytes))
        return out

    def pick(self, x, y, w=1, h=1, cap=None):
        """Distinct (object, instance) winners in the rectangle: (abi.Hit array of min(total, cap), total)."""
        n = C.c_uint32()
        if cap is None:
            self._chk(self.L.zr_pick(self.h, x, y, w, h, None, 0, C.byref(n)))
            cap = n.value
        hits = np.zeros(cap, dtype=abi.Hit)
        self._chk(self.L.zr_pick(self.h, x, y, w, h, _ptr(hits) if cap else None, cap, C.byref(n)))
        return hits[:min(cap, n.value)], n.value

    def instance_slots(self):
        """The first instance slot of every object (add order) and the slot count: one slot per instance, one per non-instanced object."""
        base, k = [], 0
        for i in range(self.object_count()):
            _, inst = self.object_get_instances(i)
            base.append(k)
            k += max(1, 0 if inst is None else len(inst))
        return np.array(base, dtype=np.int64), k

    def instance_coverage(self):
        """Pixels each instance slot won in the last frame (uint32 per slot)."""
        out = np.zeros(self.instance_slots()[1], dtype=np.uint32)
        self._chk(self.L.zr_instance_coverage(self.h, _ptr(out) if out.size else None, out.nbytes))
        return out

    def instance_coverage_async(self, dev_ptr, n_slots=None):
        """The same counts into a device buffer (address) of n_slots uint32, on the render stream, without a host sync."""
        if n_slots is None:
            n_slots = self.instance_slots()[1]
        self._chk(self.L.zr_instance_coverage_async(self.h, C.c_void_p(dev_ptr) if dev_ptr else None, 4 * n_slots))

    # ---- casting rays into the scene of the last frame
    def raycast(self, rays, flags=0):
        """The nearest hit of each ray (abi.RAY array, abi.make_rays) in the scene as the frame enqueued last drew it -> abi.RAY_RECORD array.
        flags: abi.RAY_CULL_BACK | RAY_ANY_HIT | RAY_NO_BOUNDS."""
        rays = _rays(rays)
        hits = np.zeros(len(rays), dtype=abi.RAY_RECORD)
        self._chk(self.L.zr_raycast(self.h, _ptr(rays), len(rays), flags, _ptr(hits), hits.nbytes))
        return hits

    def raycast_async(self, rays_dev, hits_dev, n, flags=0):
        """The same from n rays at the device address rays_dev into n records at hits_dev (both 16-byte aligned), on the render stream,
        without a host sync."""
        self._chk(self.L.zr_raycast_async(self.h, C.c_void_p(rays_dev) if rays_dev else None, n, flags, C.c_void_p(hits_dev) if hits_dev else None))

    def camera_ray(self, px, py):
        """The world-space ray of the uniforms set last through frame position (px, py) (pixel centres at +0.5) -> abi.RAY array of one"""
        r = abi.Ray()
        self._chk(self.L.zr_camera_ray(self.h, px, py, C.byref(r)))
        out = np.zeros(1, dtype=abi.RAY)
        out["origin"], out["dir"], out["t_min"], out["t_max"] = tuple(r.origin), tuple(r.dir), r.t_min, r.t_max
        return out

    # ---- multi-GPU
    def tiles_device_buffer(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._chk(self.L.zr_tiles_device_buffer(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def set_tiles_buffer(self, dev_ptr):
        self._chk(self.L.zr_set_tiles_buffer(self.h, C.c_void_p(dev_ptr) if dev_ptr else None))

    def read_tiles(self):
        _, nbytes = self.tiles_device_buffer()
        out = np.zeros((nbytes // (abi.TILE * abi.TILE * 4), abi.TILE, abi.TILE, 4), dtype=np.uint8)
        self._chk(self.L.zr_read_tiles(self.h, _ptr(out), out.nbytes))
        return out

    def composite(self, gathered_dev_ptr):
        self._chk(self.L.zr_composite(self.h, C.c_void_p(gathered_dev_ptr)))

    def color_device_ptr(self):
        p = C.c_void_p()
        self._chk(self.L.zr_color_device_ptr(self.h, C.byref(p)))
        return p.value

    def dist_init(self, unique_id, rank, world, split_shadow=False):
        """Native multi-GPU host: the library calls RCCL itself (zr_dist_frame = render + all-gather + composite).
        split_shadow: False / "replicated", True / "split", or "tiles" (abi.SHADOW_MODES)."""
        self._dist_id = bytes(unique_id)
        self._chk(self.L.zr_dist_init(self.h, self._dist_id, len(self._dist_id), rank, world, abi.dist_flags(abi.shadow_mode(split_shadow))))

    def dist_prepare(self, rank, world, split_shadow=False):
        """The local half of dist_init (librccl, collective stream, buffers): safe to fail on one rank alone."""
        self._chk(self.L.zr_dist_prepare(self.h, rank, world, abi.dist_flags(abi.shadow_mode(split_shadow))))

    def dist_connect(self, unique_id):
        """ncclCommInitRank: a collective - call it only when every rank's dist_prepare succeeded."""
        self._dist_id = bytes(unique_id)
        self._chk(self.L.zr_dist_connect(self.h, self._dist_id, len(self._dist_id)))

    def dist_frame(self):
        self._chk(self.L.zr_dist_frame(self.h))

    def dist_copy_frame_async(self, color_dev_ptr):
        """zr_dist_copy_frame_async: the last enqueued frame's composite into a caller-owned device buffer, in collective-stream order."""
        self._chk(self.L.zr_dist_copy_frame_async(self.h, C.c_void_p(color_dev_ptr)))

    # ---- world / livelink
    def profab_register(self, name, mesh, material=None):
        mat = C.cast(C.pointer(material), C.c_void_p) if material is not None else None
        self._chk(self.L.zr_profab_register(self.h, name.encode(), mesh, mat))

    def world_load_json(self, text):
        b = text.encode() if isinstance(text, str) else bytes(text)
        self._chk(self.L.zr_world_load_json(self.h, b, len(b)))

    def world_update_json(self, text):
        """zr_world_update_json: the payload applied as a difference from the live scene; returns zr_world_delta as a dict
        (differs, scene_changed, objects_kept, objects_reinstanced, objects_added, objects_removed, materials_rebuilt, history_items)."""
        b = text.encode() if isinstance(text, str) else bytes(text)
        d = abi.WorldDelta()
        self._chk(self.L.zr_world_update_json(self.h, b, len(b), C.byref(d), C.sizeof(d)))
        return _delta_dict(d)

    def world_update_file(self, path=None):
        d = abi.WorldDelta()
        self._chk(self.L.zr_world_update_file(self.h, os.fsencode(path) if path is not None else None, C.byref(d), C.sizeof(d)))
        return _delta_dict(d)

    def livelink_set_incremental(self, on=True):
        """zr_livelink_poll applies payloads with zr_world_update_json instead of zr_world_load_json."""
        self._chk(self.L.zr_livelink_set_incremental(self.h, int(bool(on))))

    def set_asset_root(self, path):
        """The engine's working directory (Profabs/, Content/): world loads then resolve Profabs and sky / cubemap / background files."""
        self._chk(self.L.zr_set_asset_root(self.h, os.fsencode(path) if path is not None else None))

    def asset_path_search(self, name):
        n = C.c_size_t()
        self._chk(self.L.zr_asset_path_search(self.h, name.encode(), None, 0, C.byref(n)))
        buf = C.create_string_buffer(max(1, n.value))
        self._chk(self.L.zr_asset_path_search(self.h, name.encode(), buf, n.value, C.byref(n)))
        return buf.raw[:n.value].decode()

    def load_meshlet_file(self, path):
        m = C.c_uint32()
        self._chk(self.L.zr_load_meshlet_file(self.h, os.fsencode(path), C.byref(m)))
        return m.value

    def world_load_file(self, path=None):
        self._chk(self.L.zr_world_load_file(self.h, os.fsencode(path) if path is not None else None))

    def world_save_file(self, path=None):
        self._chk(self.L.zr_world_save_file(self.h, os.fsencode(path) if path is not None else None))

    def world_update_uniforms(self, roll_stage=0.0, roll_light=0.0, time=0.0):
        self._chk(self.L.zr_world_update_uniforms(self.h, roll_stage, roll_light, time))

    def world_save_json(self):
        n = C.c_size_t()
        self._chk(self.L.zr_world_save_json(self.h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        self._chk(self.L.zr_world_save_json(self.h, buf, n.value, C.byref(n)))
        return buf.raw[:n.value].decode()

    def world_camera(self):
        cam = abi.Camera()
        self._chk(self.L.zr_world_get_camera(self.h, C.cast(C.pointer(cam), C.c_void_p)))
        return cam

    def livelink_serve(self, port=8080, bind_any=False):
        self._chk(self.L.zr_livelink_bind_any(self.h, int(bind_any)))
        self._chk(self.L.zr_livelink_serve(self.h, port))
        p = C.c_uint16()
        self._chk(self.L.zr_livelink_port(self.h, C.byref(p)))
        return p.value

    def livelink_poll(self):
        r = C.c_int()
        self._chk(self.L.zr_livelink_poll(self.h, C.byref(r)))
        return bool(r.value)

    def livelink_stop(self):
        self._chk(self.L.zr_livelink_stop(self.h))


def load_scene(r, cfg):
    """Feed a scenes.config*() dict to a Renderer."""
    r.set_cubemap(cfg.get("cubemap"))
    for o in cfg["objects"]:
        m = r.mesh_create(*o["mesh"])
        r.object_add(m, o.get("material"), o.get("instances"))
    r.update_uniforms(cfg["camera"], cfg["dir"], cfg["point"], cfg["spot"])
