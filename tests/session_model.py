"""Seeded sessions of updates, rests and deliveries, and the state model that tells what each frame and each delivery must hold.

TEST INFRASTRUCTURE: numpy only, no GPU.  Three pieces:

  Model      everything a frame and its deliveries depend on, as plain values: extent, the four objects' data, camera, lights, the
             lighting pass's switches, the highlight set, the overlay list, the delta stream and the client's copy.  `populate` builds
             the scene from scratch on a renderer or on the oracle (which knows no visibility: what is hidden is left out of its scene),
             `uniforms` sets a frame's uniforms, `apply` performs one operation on the model and, when given one, on a renderer.
  script     seed -> a list of steps.  A step is a dict of plain values - {"ops": [(kind, k), ..], "entry", "advance", "sync",
             "readers": [(kind, k), ..]} - so that a failing session can be printed, pasted and cut down by hand.
  run        plays steps against the oracle and, when given one, a renderer; what is compared, and how, is the caller's (`Hooks`).

Rest depth of a frame: the number of consecutive frames before it whose camera-pass and surface inputs were its own (0 after a change).
An operation "falls at" the depth class (0, 1, 2, 3 = three or more) of the frame before its gap.

The scene is dyadic where a ray cast has to be byte-equal to the host statement: instances have no rotation, power-of-two scales and
positions on an eighth's grid, so a world corner is p * s + t with one rounding whatever the order of operations - while roll_stage is 0.
Ray casts are therefore drawn only while the stage is not rolled; every other reader is drawn in every state that allows it.
"""
import numpy as np

import frame_delta_reference as fdr
import frame_scale_reference as fsr
import highlight_reference as hr
import ids_reference as idr
import overlay_reference as ovr
from zeldaengine_amd import abi, scenes

PLANE, BOX, SPHERES, TERRAIN, EXTRA = 0, 1, 2, 3, 4          # object indices = mesh ids, in add order
N_INST = 120
REST_ARG_LIGHTS = 64                                         # ZR_REST_ARG_LIGHTS (csrc/zr_types.h)
EXTENTS = ((96, 64), (160, 90), (33, 17))
CAMS = (((9.0, -7.0, 6.0), (0.0, 0.0, 1.0)), ((7.0, 6.0, 5.0), (0.0, 0.0, 0.5)), ((-8.0, -5.0, 7.0), (0.0, 0.0, 1.0)), ((3.0, -10.0, 4.0), (0.0, 0.0, 1.0)))
SUNS = ((6.0, 0.0, 14.0), (5.0, 2.0, 13.0), (4.0, -3.0, 12.0))
LIGHT_COUNTS = (2, 16, 0, REST_ARG_LIGHTS + 1)
VIEWS = (0, 2, 5, 6, 8)                                      # (view 9 reads XkView behind the pass and is not the oracle's)
ENTRIES = ("render", "staged", "geometry")
HL_STYLES = ("opaque", "half", "fill")

# operation kind -> family.  camera / scene / surface operations end a rest (the camera pass's or the resolve's inputs change); light
# operations move only what the lighting pass reads; delivery operations move no frame at all.
FAMILY = {
    "camera_jump": "camera", "camera_ulp": "camera", "roll_stage": "camera",
    "sun_move": "light", "light_count": "light", "set_background": "light", "set_cubemap": "light", "set_debug_view": "light",
    "set_instances": "scene", "update_instances_async": "scene", "set_vertices_sphere": "scene", "update_vertices_sphere_async": "scene",
    "set_vertices_terrain": "scene", "update_vertices_terrain_async": "scene", "set_instance_visibility": "scene",
    "update_instance_visibility_async": "scene", "object_hide": "scene", "object_show": "scene", "object_add": "scene",
    "scene_clear": "scene", "set_limits": "scene", "resize": "scene",
    "set_texture": "surface", "update_texture_async": "surface", "id_capture_on": "surface", "id_capture_off": "surface",
    "shading_forward": "surface", "shading_back": "surface",
    "highlight_set": "delivery", "highlight_clear": "delivery", "overlay_set": "delivery", "overlay_clear": "delivery",
    "delta_on": "delivery", "delta_off": "delivery", "delta_reset": "delivery", "delta_scale": "delivery",
}
OP_KINDS = tuple(FAMILY)
ENDS_REST = ("camera", "scene", "surface")
# the target an operation must move on the oracle (tests/test_session_model.py): the shadow map for caster changes, a GBuffer plane for
# camera and surface changes, colour for lighting-side ones; None: the operation moves no frame (or changes its shape)
MOVES = {k: {"camera": "gbuffer", "scene": "shadow", "surface": "gbuffer", "light": "color", "delivery": None}[f] for k, f in FAMILY.items()}
# (one ulp of View is there because it moves the camera pass's key and, at these extents, no pixel: it is held to no target)
MOVES.update({"camera_ulp": None, "sun_move": "shadow", "set_limits": None, "resize": None, "id_capture_on": None, "id_capture_off": None, "shading_forward": "color",
              "shading_back": "color"})
ASYNC = tuple(k for k in OP_KINDS if k.endswith("_async"))
HOST_READERS = ("color_scaled", "color_highlighted", "read_color_overlaid", "read_frame_delta", "read_frame_delta_packed", "read_ids", "pick",
                "instance_coverage", "raycast")
DEVICE_READERS = ("copy_frame_scaled_async", "instance_coverage_async", "raycast_async")
READER_KINDS = ("frame", "copy_frame_async") + HOST_READERS + DEVICE_READERS      # "frame": colour, the six GBuffer planes, the shadow map


def _lights(n):
    w = scenes.sample_world()
    d, _, s = scenes.lights_from_world(w)
    w["PointLights"] = scenes.sample_point_lights(n)
    _, p, _ = scenes.lights_from_world(w)
    return d, p, s


def _instances(k):
    """N_INST dyadic instance records: no rotation, scales 1/4 .. 1, positions on the 1/8 grid"""
    rng = np.random.default_rng(1000 + k)
    out = np.zeros(N_INST, dtype=abi.XkInstanceData)
    out["InstancePosition"][:, :2] = rng.integers(-48, 49, (N_INST, 2)) / 8.0
    out["InstancePosition"][:, 2] = rng.integers(2, 21, N_INST) / 8.0
    out["InstancePScale"] = np.array([0.25, 0.5, 1.0], dtype=np.float32)[rng.integers(0, 3, N_INST)]
    return out


def _image(k, dim):
    rng = np.random.default_rng(2000 + k)
    img = rng.integers(0, 256, (dim, dim, 4), dtype=np.uint8)
    img[..., 3] = 255
    return img


def _cube(k):
    faces = scenes.synthetic_cubemap(16 if k % 2 == 0 else 8)
    return faces if k % 4 < 2 else [255 - f for f in faces]


def _segments(k):
    """a box round the scene's middle, a diagonal through the ground (hidden parts) and an x-ray axis"""
    rng = np.random.default_rng(3000 + k)
    c = rng.integers(-16, 17, 3) / 8.0 + (0.0, 0.0, 2.0)
    h = 1.5
    rows = []
    for a, b in (((-h, -h, -h), (h, -h, -h)), ((h, -h, -h), (h, h, -h)), ((h, h, -h), (-h, h, -h)), ((-h, h, -h), (-h, -h, -h)),
                 ((-h, -h, -h), (-h, -h, h)), ((h, h, -h), (h, h, h)), ((-h, -h, h), (h, h, h))):
        rows.append(tuple(c + a) + tuple(c + b) + (255, 40 + 20 * k % 200, 0, 255))
    rows.append((-6.0, -6.0, -1.0, 6.0, 6.0, 3.0, 0, 255, 200, 160))
    rows.append((0.0, 0.0, 0.0, 0.0, 0.0, 5.0, 30, 60, 255, 200, abi.OVERLAY_XRAY))
    return abi.make_overlay_segments(rows)


def start(seed):
    """What a session starts from, each drawn on its own from the seed's generator: the context's flavour (half the seeds the default
    one), extent, shadow size, light count, id capture, the box's image size, what the first gap sets up, whether a stretch without
    host synchronisation is put in"""
    rng = np.random.default_rng(30000 + seed)
    flags, sky = ((0, False), (0, False), (0, False), (abi.FLAG_SERIAL_PASSES, False), (abi.FLAG_NO_LIST_REUSE, False), (0, True))[int(rng.integers(0, 6))]
    return {"flags": flags, "sky": sky, "extent": EXTENTS[int(rng.integers(0, 2))], "SD": (64, 128)[int(rng.integers(0, 2))],
            "n_point": LIGHT_COUNTS[int(rng.integers(0, 2))], "capture": bool(rng.integers(0, 2)), "big_image": int(rng.integers(0, 8)) == 0,
            "first": int(rng.integers(0, 3)), "stretch": int(rng.integers(0, 3)) != 0}


class Model:
    def __init__(self, seed=0):
        st = start(seed)
        self.seed, self.sky = seed, st["sky"]
        self.W, self.H = st["extent"]
        self.SD = st["SD"]
        self.big_image = st["big_image"]                     # a 192 x 192 image: the smallest above a staging slot's first capacity
        self.inst, self.mask = _instances(seed), np.ones(N_INST, dtype=bool)
        self.sphere, self.sphere_idx = scenes.uv_sphere(8, 5)
        self.terrain, self.terrain_idx = scenes.grid_plane(6.0, 12, 0.02)
        self.sphere0, self.terrain0 = self.sphere.copy(), self.terrain.copy()
        self.box_image = _image(seed, 192 if self.big_image else 16)
        self.box_shown, self.extra = True, False
        self.cam, self.ulps, self.sun, self.n_point = 0, 0, 0, st["n_point"]
        self.tick, self.roll_stage = 0, 0.0
        self.view, self.bg, self.cube, self.forward, self.capture = 0, None, 0, False, st["capture"]
        self.highlight, self.hl_style, self.hl_radius = np.zeros(self.slots()[1], dtype=np.uint8), "opaque", 2
        self.overlay, self.ov_style = None, {"depth_bias": 0.0, "hidden_opacity": 0}
        self.delta, self.delta_scale, self.client, self.delta_full = 0, 1, None, True
        self.limits = 0
        self.version = 0                                    # of everything the oracle's scene is built from
        self._keep = []
        # what the readers may ask of the frame enqueued last
        self.have_frame, self.frame_captured, self.scene_changed = False, False, False
        self.frame_state = None                             # the frame's own copies of what rays and lines see

    # ---- the scene
    def slots(self):
        counts = [1, 1, N_INST, 1] + ([1] if self.extra else [])
        return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64), int(sum(counts))

    def populate(self, r, oracle=False):
        """the scene from scratch; on a renderer the hidden parts are added and then hidden, the oracle never sees them"""
        r.set_cubemap(_cube(self.cube))
        r.object_add(r.mesh_create(*scenes.grid_plane(60.0, 8, 0.0)))
        if self.box_shown or not oracle:
            mat, keep = abi.make_material([self.box_image] + [None] * 6)
            self._keep.append(keep)
            r.object_add(r.mesh_create(*scenes.box((1.0, 1.0, 0.75), (3.0, -2.0, 0.75))), mat)
        inst = self.inst[self.mask] if oracle else self.inst
        r.object_add(r.mesh_create(self.sphere, self.sphere_idx), None, inst)
        r.object_add(r.mesh_create(self.terrain, self.terrain_idx))
        if self.extra:
            r.object_add(r.mesh_create(*scenes.box((1.0, 1.0, 1.0), (-2.0, 1.0, 3.0))))
        if self.sky:
            r.set_skydome(*scenes.sky_dome(20.48, 16, 8), scenes.synthetic_sky_image(64, 32))
        if self.bg is not None:
            r.set_background(scenes.synthetic_sky_image(48 + 16 * (self.bg % 2), 32))
        if not oracle:
            if not self.box_shown:
                r.object_set_visible(BOX, False)
            if not self.mask.all():
                r.object_set_instance_visibility(SPHERES, self.mask)

    def uniforms(self, r, i=None):
        """the frame's uniforms; roll_light and time follow the model's tick (i: another tick), which stands while the lights do"""
        i = self.tick if i is None else i
        d, p, s = _lights(self.n_point)
        sun = SUNS[self.sun]
        d[0]["Position"][:3] = sun; d[0]["Direction"][:3] = sun
        r.update_uniforms(abi.make_camera(*CAMS[self.cam], fov=50.0), d, p, s, self.roll_stage, 0.05 * i, 1.0 + 0.1 * i)
        if self.ulps:
            cam, sh, view = r.get_frame()
            v = np.float32(cam["View"][12])
            for _ in range(self.ulps):
                v = np.nextafter(v, np.float32(np.inf))
            cam["View"][12] = v
            r.set_frame(cam, sh, view)

    def oracle_items(self):
        """(items of ids_reference for the oracle's scene, the renderer's object index of each, the renderer's instance index of each
        shown sphere)"""
        items, objs = [(128, None)], [PLANE]
        if self.box_shown:
            items.append((12, None)); objs.append(BOX)
        shown = np.flatnonzero(self.mask)
        items.append((len(self.sphere_idx) // 3, shown)); objs.append(SPHERES)
        items.append((len(self.terrain_idx) // 3, None)); objs.append(TERRAIN)
        if self.extra:
            items.append((12, None)); objs.append(EXTRA)
        return items, np.array(objs, dtype=np.uint32), shown.astype(np.uint32)

    def object_plane(self, vis):
        """zr_read_ids(ZR_IDS_OBJECT) from the oracle's visibility buffer: ids_reference's plane, renumbered to the full scene"""
        items, objs, shown = self.oracle_items()
        pl = idr.object_plane(vis, items)
        none = pl[..., 0] == idr.NO_ID
        o = objs[np.where(none, 0, pl[..., 0])]
        spheres = ~none & (o == SPHERES)
        inst = np.where(spheres, shown[np.where(spheres, pl[..., 1], 0)] if len(shown) else 0, pl[..., 1])
        return np.stack([np.where(none, idr.NO_ID, o), np.where(none, idr.NO_ID, inst)], axis=-1).astype(np.uint32)

    def coverage(self, vis):
        pl = self.object_plane(vis)
        base, n = self.slots()
        s = hr.slots_of(pl, base)
        return np.bincount(s[s >= 0], minlength=n).astype(np.uint32)

    def pick(self, vis, depth, x, y, w, h):
        items, objs, shown = self.oracle_items()
        hits, total = idr.pick(vis, depth, items, x, y, w, h)
        return [(int(objs[t[0]]), int(shown[t[1]]) if objs[t[0]] == SPHERES else t[1]) + t[2:] for t in hits], total

    def world_triangles(self):
        """the shown world triangles in draw order (non-instanced draws first) as float32 corners, and who each is: (object, instance,
        triangle) - exact while the stage is not rolled"""
        assert self.roll_stage == 0.0
        tris, who = [], []

        def add(obj, verts, idx, inst, k):
            p = np.asarray(verts["Position"], dtype=np.float32)[np.asarray(idx, dtype=np.int64).reshape(-1, 3)]
            if inst is not None:
                p = p * np.float32(inst["InstancePScale"]) + inst["InstancePosition"].astype(np.float32)
            tris.append(p.astype(np.float32))
            who.append(np.stack([np.full(len(p), obj), np.full(len(p), k), np.arange(len(p))], axis=1))
        add(PLANE, *scenes.grid_plane(60.0, 8, 0.0), None, 0)
        if self.box_shown:
            add(BOX, *scenes.box((1.0, 1.0, 0.75), (3.0, -2.0, 0.75)), None, 0)
        add(TERRAIN, self.terrain, self.terrain_idx, None, 0)
        if self.extra:
            add(EXTRA, *scenes.box((1.0, 1.0, 1.0), (-2.0, 1.0, 3.0)), None, 0)
        for k in np.flatnonzero(self.mask):
            add(SPHERES, self.sphere, self.sphere_idx, self.inst[k], int(k))
        return np.concatenate(tris), np.concatenate(who).astype(np.uint32)

    def free_rays(self, k):
        """a fan from the camera that runs over the scene and past it into the sky, and a few rays of no camera"""
        rng = np.random.default_rng(4000 + k)
        pos, look = np.array(CAMS[self.cam][0]), np.array(CAMS[self.cam][1])
        aim = look + np.stack([rng.uniform(-9, 9, 24), rng.uniform(-9, 9, 24), rng.uniform(-1.0, 9.0, 24)], axis=1)
        rays = [abi.make_rays(np.tile(pos, (24, 1)), aim - pos, 0.0, np.inf)]
        o = np.stack([rng.integers(-40, 41, 8) / 8.0, rng.integers(-40, 41, 8) / 8.0, np.full(8, 6.0)], axis=1)
        d = np.tile((0.0, 0.0, -1.0), (8, 1)); d[6:] = (0.0, 0.0, 1.0)
        rays.append(abi.make_rays(o, d, 0.0, np.inf))
        return np.concatenate(rays)

    def expect_rays(self, engine, rays, frame_state):
        """zr_ray_triangles over the frame's shown triangles, its records renamed (object, instance, triangle)"""
        tris, who = frame_state
        h = engine.ray_triangles(rays, tris, 0)
        m = h["object"] != idr.NO_ID
        w = who[h["triangle"][m]]
        h["object"][m], h["instance"][m], h["triangle"][m] = w[:, 0], w[:, 1], w[:, 2]
        return h

    # ---- operations
    def _scene_op(self):
        self.version += 1

    def apply(self, op, r=None, dev=None):
        """one operation on the model and, when given, on renderer r.  dev(array, row_bytes) -> a device tensor (the caller keeps it
        alive while the update is in flight)"""
        kind, k = op
        fam = FAMILY[kind]
        if kind == "camera_jump":
            self.cam = (self.cam + 1 + k % 3) % len(CAMS); self.ulps = 0
        elif kind == "camera_ulp":
            self.ulps += 1 + k % 2
        elif kind == "roll_stage":
            self.roll_stage = 0.3 if self.roll_stage == 0.0 else 0.0
        elif kind == "sun_move":
            self.sun = (self.sun + 1 + k % 2) % len(SUNS)
        elif kind == "light_count":
            self.n_point = LIGHT_COUNTS[(LIGHT_COUNTS.index(self.n_point) + 1 + k % 3) % len(LIGHT_COUNTS)]
        elif kind == "set_background":
            self.bg = 0 if self.bg is None else self.bg + 1
            self._scene_op()
            if r:
                r.set_background(scenes.synthetic_sky_image(48 + 16 * (self.bg % 2), 32))
        elif kind == "set_cubemap":
            self.cube += 1 + k % 3
            self._scene_op()
            if r:
                r.set_cubemap(_cube(self.cube))
        elif kind == "set_debug_view":
            self.view = VIEWS[(VIEWS.index(self.view) + 1 + k % 4) % len(VIEWS)]
            if r:
                r.set_debug_view(self.view)
        elif kind in ("set_instances", "update_instances_async"):
            new = _instances(100 + k)
            first, n = (0, N_INST) if k % 2 else (N_INST // 4, N_INST // 2)
            self.inst = self.inst.copy(); self.inst[first:first + n] = new[first:first + n]
            self._scene_op()
            if r and kind == "set_instances":
                r.object_set_instances(SPHERES, self.inst[first:first + n], first=first)
            elif r:
                r.object_update_instances_async(SPHERES, dev(self.inst[first:first + n], 32), first=first)
        elif kind in ("set_vertices_sphere", "update_vertices_sphere_async"):
            v = self.sphere0.copy()
            v["Position"][:, 2] *= np.float32(1.0 + 0.25 * (1 + k % 3)); v["Position"][:, 0] *= np.float32(1.0 - 0.125 * (k % 2))
            if np.array_equal(v["Position"], self.sphere["Position"]):
                v["Position"][:, 1] *= np.float32(1.5)
            self.sphere = v
            self._scene_op()
            if r and kind == "set_vertices_sphere":
                r.mesh_set_vertices(SPHERES, v)
            elif r:
                r.mesh_update_vertices_async(SPHERES, dev(v, 44))
        elif kind in ("set_vertices_terrain", "update_vertices_terrain_async"):
            v = self.terrain0.copy()
            x, y = v["Position"][:, 0], v["Position"][:, 1]
            v["Position"][:, 2] = (0.02 + (0.3 + 0.2 * (k % 3)) * (1.0 + np.sin(1.3 * x + k) * np.cos(0.9 * y))).astype(np.float32)
            if np.array_equal(v["Position"], self.terrain["Position"]):
                v["Position"][:, 2] += np.float32(0.25)
            self.terrain = v
            self._scene_op()
            if r and kind == "set_vertices_terrain":
                r.mesh_set_vertices(TERRAIN, v)
            elif r:
                r.mesh_update_vertices_async(TERRAIN, dev(v, 44))
        elif kind in ("set_instance_visibility", "update_instance_visibility_async"):
            new = np.random.default_rng(5000 + k).random(N_INST) > 0.4
            if np.array_equal(new, self.mask):
                new = ~new
            self.mask = new
            self._scene_op()
            if r and kind == "set_instance_visibility":
                r.object_set_instance_visibility(SPHERES, new)
            elif r:
                r.object_update_instance_visibility_async(SPHERES, dev(new.astype(np.uint8), 1))
        elif kind in ("object_hide", "object_show"):
            self.box_shown = kind == "object_show"
            self._scene_op()
            if r:
                r.object_set_visible(BOX, self.box_shown)
        elif kind == "object_add":
            assert not self.extra
            self.extra = True
            self.highlight = np.zeros(self.slots()[1], dtype=np.uint8)      # (the set is cleared whenever the object list changes)
            self._scene_op(); self.scene_changed = True
            if r:
                r.object_add(r.mesh_create(*scenes.box((1.0, 1.0, 1.0), (-2.0, 1.0, 3.0))))
        elif kind == "scene_clear":
            self.inst, self.mask, self.box_shown, self.extra = _instances(200 + k), np.ones(N_INST, dtype=bool), True, False
            self.sphere, self.terrain = self.sphere0.copy(), self.terrain0.copy()
            self.highlight = np.zeros(self.slots()[1], dtype=np.uint8)
            self._scene_op(); self.scene_changed = True
            if r:
                r.scene_clear(); self.populate(r)
        elif kind == "set_limits":
            self.limits = (self.limits + 1) % 2
            if r:
                r.set_limits(*((8192, 4096) if self.limits else (0, 0)))
        elif kind == "resize":
            e = [x for x in EXTENTS if x != (self.W, self.H)][k % 2]
            self.W, self.H = e
            self._scene_op()
            self.have_frame = False                          # until the next frame the readers answer as on a new context
            if self.delta:
                self.client, self.delta_full = self._client(), True
            if r:
                r.resize(*e)
        elif kind in ("set_texture", "update_texture_async"):
            self.box_image = _image(300 + k, self.box_image.shape[0])
            self._scene_op()
            if r and kind == "set_texture":
                r.object_set_texture(BOX, 0, self.box_image)
            elif r:
                r.object_update_texture_async(BOX, 0, dev(self.box_image, None))
        elif kind in ("id_capture_on", "id_capture_off"):
            self.capture = kind == "id_capture_on"
            if r:
                r.set_id_capture(self.capture)
        elif kind in ("shading_forward", "shading_back"):
            self.forward = kind == "shading_forward"
            if r:
                r.set_shading(self.forward)
        elif kind == "highlight_set":
            rng = np.random.default_rng(6000 + k)
            on = (rng.random(N_INST) < 0.3).astype(np.uint8)
            base, _ = self.slots()
            self.highlight[base[SPHERES]:base[SPHERES] + N_INST] = on
            self.highlight[base[BOX]] = k % 2
            self.hl_style, self.hl_radius = HL_STYLES[k % 3], 1 + k % 4
            if r:
                r.highlight_set(SPHERES, on); r.highlight_set(BOX, k % 2)
                r.set_highlight_style(**hr.style(self.hl_style, self.hl_radius))
        elif kind == "highlight_clear":
            self.highlight[:] = 0
            if r:
                r.highlight_clear()
        elif kind == "overlay_set":
            self.overlay = k
            self.ov_style = {"depth_bias": 0.0 if k % 2 else 0.001, "hidden_opacity": (0, 96)[k % 2]}
            if r:
                r.overlay_set(_segments(k)); r.overlay_style(abi.make_overlay_style(**self.ov_style))
        elif kind == "overlay_clear":
            self.overlay = None
            if r:
                r.overlay_set(None)
        elif kind == "delta_on":
            self.delta = abi.FRAME_DELTA_PACKED if k % 2 else 1
            self.client, self.delta_full = self._client(), True
            if r:
                r.set_frame_delta(self.delta)
        elif kind == "delta_off":
            self.delta, self.client = 0, None
            if r:
                r.set_frame_delta(False)
        elif kind == "delta_reset":
            self.client, self.delta_full = self._client(), True
            if r:
                r.frame_delta_reset()
        elif kind == "delta_scale":                          # (only while delta is off: off, the scale, on again)
            was = self.delta
            self.delta_scale = 1 + (self.delta_scale + k % 2) % 3
            if r and was:
                r.set_frame_delta(False)
            if r:
                r.set_frame_delta_scale(self.delta_scale)
            if was:
                self.client, self.delta_full = self._client(), True
                if r:
                    r.set_frame_delta(was)
        else:
            raise ValueError(kind)
        return fam

    def _client(self):
        h, w = -(-self.H // self.delta_scale), -(-self.W // self.delta_scale)
        return np.zeros((h, w, 4), dtype=np.uint8)

    def allowed(self, kind):
        """whether the operation can be applied in this state, between frames (the device forms need a scene a frame has drawn)"""
        if kind in ASYNC:
            return self.have_frame and not self.scene_changed and (kind != "update_texture_async" or self.box_shown)
        return {"object_hide": self.box_shown, "object_show": not self.box_shown, "object_add": not self.extra,
                "id_capture_on": not self.capture, "id_capture_off": self.capture, "shading_forward": not self.forward,
                "shading_back": self.forward, "highlight_clear": bool(self.highlight.any()), "overlay_clear": self.overlay is not None,
                "delta_on": not self.delta, "delta_off": bool(self.delta), "delta_reset": bool(self.delta), "set_texture": self.box_shown,
                }.get(kind, True)

    def reader_allowed(self, kind):
        """whether the reader has an answer for the frame enqueued last"""
        ids = self.frame_captured and not self.scene_changed
        if kind in ("read_ids", "pick", "instance_coverage", "instance_coverage_async"):
            return ids
        if kind in ("raycast", "raycast_async"):
            return self.roll_stage == 0.0 and not self.scene_changed
        if kind == "read_frame_delta":
            return bool(self.delta)
        if kind == "read_frame_delta_packed":
            return self.delta == abi.FRAME_DELTA_PACKED
        if kind == "read_color_overlaid":
            return self.overlay is not None
        if kind == "color_highlighted":
            return ids and bool(self.highlight.any())
        return True

    def frame_done(self):
        """a frame of the current state has been enqueued"""
        self.have_frame, self.frame_captured, self.scene_changed = True, self.capture, False
        self.frame_state = self.world_triangles() if self.roll_stage == 0.0 else None

    # ---- what the deliveries must hold, from the oracle's frame of the same state
    def highlighted(self, color, vis):
        mask = hr.mask_of(self.object_plane(vis), self.highlight, self.slots()[0])
        return hr.highlight(color, mask, hr.style(self.hl_style, self.hl_radius))

    def overlaid(self, o, color):
        mvp = o.get_frame()[0]
        pvm = ovr.pvm_of(mvp["Proj"], mvp["View"], mvp["Model"])
        return ovr.overlay(color, o.gbuffer(0).astype(np.float32), pvm, _segments(self.overlay), self.ov_style)

    def delivery(self, color):
        """-> (tiles, pixels, full, frame delivered): the next delivery of changes; the client's copy takes it"""
        f = color if self.delta_scale == 1 else fsr.downscale(color, self.delta_scale)
        full = self.delta_full
        tiles, pixels = fdr.delta(self.client, f, full)
        fdr.apply(self.client, tiles, pixels)
        self.delta_full = False
        return tiles, pixels, full, f


def expect(reader, m, o, engine=None, rays=None):
    """what the reader must return for the frame the oracle o holds, by the reader's own statement (a delivery of changes moves the
    model's client copy: once per delivery)"""
    kind, k = reader
    color = o.color()
    if kind in ("color_scaled", "copy_frame_scaled_async"):
        return fsr.downscale(color, reader_scale(reader))
    if kind == "color_highlighted":
        out = m.highlighted(color, o.visibility())
        return out if reader_scale(reader) == 1 else fsr.downscale(out, reader_scale(reader))
    if kind == "read_color_overlaid":
        out = m.overlaid(o, color)
        return out if reader_scale(reader) == 1 else fsr.downscale(out, reader_scale(reader))
    if kind in ("read_frame_delta", "read_frame_delta_packed"):
        return m.delivery(color)
    if kind == "read_ids":
        return m.object_plane(o.visibility())
    if kind in ("instance_coverage", "instance_coverage_async"):
        return m.coverage(o.visibility())
    if kind == "pick":
        return m.pick(o.visibility(), o.gbuffer(0), *pick_rect(reader, o.visibility()))
    if kind in ("raycast", "raycast_async"):
        return m.expect_rays(engine, rays, m.frame_state)
    raise ValueError(kind)


def reader_scale(reader):
    kind, k = reader
    return 2 + k % 3 if kind in ("color_scaled", "copy_frame_scaled_async") else 1 + k % 2


def pick_rect(reader, vis):
    """a rectangle of 1 x 1 to 40 x 23 pixels that holds a covered pixel of the frame (vis: the oracle's visibility buffer)"""
    k = reader[1]
    ys, xs = np.nonzero(vis != idr.NO_ID)
    j = (k * 7919) % len(xs)
    w, h = 1 + k % 40, 1 + k % 23
    return max(0, int(xs[j]) - k % w), max(0, int(ys[j]) - k % h), w, h


class Rest:
    """rest depth as the model counts it, and the standing of what the lighting pass and the shadow map read"""

    def __init__(self):
        self.depth = self.sun = self.light = 0              # consecutive frames so far with equal camera / shadow / lighting inputs
        self.last_class = None                              # the class of the frame enqueued last

    def gap(self, kinds, advance):
        fams = {FAMILY[k] for k in kinds}
        if fams & set(ENDS_REST):
            self.depth = self.sun = 0
        if "sun_move" in kinds:
            self.sun = 0
        if fams & {"light"} or fams & set(ENDS_REST) or advance:
            self.light = 0

    def frame(self):
        """-> (depth of this frame, frames its sun and casters stood, frames its lighting inputs stood)"""
        out = (self.depth, self.sun, self.light)
        self.last_class = min(self.depth, 3)
        self.depth += 1; self.sun += 1; self.light += 1
        return out


# ------------------------------------------------------------------------------------------------ the generator

def _cells():
    cells = [(k, d) for k in OP_KINDS for d in range(4)]
    order = np.random.default_rng(77).permutation(len(cells))
    return [cells[i] for i in order]


CELLS = _cells()
DEFAULT_SEEDS = 24
_FIXES = {"object_show": "object_hide", "id_capture_off": "id_capture_on", "shading_back": "shading_forward", "highlight_clear": "highlight_set",
          "overlay_clear": "overlay_set", "delta_off": "delta_on", "delta_reset": "delta_on", "object_hide": "object_show",
          "id_capture_on": "id_capture_off", "shading_forward": "shading_back", "delta_on": "delta_off", "object_add": "scene_clear",
          "set_texture": "object_show", "update_texture_async": "object_show", "set_background": "set_debug_view"}
_COMPANIONS = ("camera_jump", "sun_move", "set_instances", "light_count", "camera_ulp", "set_cubemap", "overlay_set", "set_vertices_terrain",
               "set_texture", "highlight_set", "set_instance_visibility", "roll_stage")


_NEEDY = ("color_highlighted", "read_frame_delta_packed", "read_color_overlaid", "read_frame_delta", "pick")


def flavour(seed):
    """(zr_config flags, created with a skydome)"""
    st = start(seed)
    return st["flags"], st["sky"]


def script(seed):
    """The session of a seed: 24 to 40 steps.  Every seed works off its share of the (operation kind x rest-depth class) cells - rests of
    the right length are put before each - and fills the rest with runs where nothing changes, where only the point lights move and where
    nothing moves at all."""
    rng = np.random.default_rng(10000 + seed)
    m, rest = Model(seed), Rest()
    steps, textured = [], 0
    share = -(-len(CELLS) // DEFAULT_SEEDS)
    targets = [CELLS[(seed * share + j) % len(CELLS)] for j in range(share + 3)]      # (overlapping: a target may have to be skipped)
    reader_turn = {(c, n): seed + 3 * c for c in range(4) for n in (len(_NEEDY), len(HOST_READERS + DEVICE_READERS), len(DEVICE_READERS))}

    def readers(sync):
        """two readers for the frame enqueued last: one of those that need a state (a set, a list, a stream, captured winners) whenever
        one is allowed, one of all - each taken in turn per depth class, so that every reader meets every class"""
        c = rest.last_class
        out = []
        for pool in ((_NEEDY, HOST_READERS + DEVICE_READERS) if sync else (DEVICE_READERS, DEVICE_READERS)):
            for _ in range(len(pool)):
                kind = pool[reader_turn[c, len(pool)] % len(pool)]
                reader_turn[c, len(pool)] += 1
                taken = [x[0] for x in out]
                if kind.startswith("read_frame_delta") and any(x.startswith("read_frame_delta") for x in taken):
                    continue                                 # (one delivery of changes per frame: a second one would list nothing)
                if m.reader_allowed(kind) and kind not in taken:
                    out.append((kind, int(rng.integers(0, 1000))))
                    break
        return out

    def step(ops, advance=None):
        for op in ops:
            m.apply(op)
        advance = bool(rng.random() < 0.5) if advance is None else advance
        rest.gap([k for k, _ in ops], advance)
        rest.frame()
        if advance:
            m.tick += 1
        m.frame_done()
        steps.append({"ops": list(ops), "entry": ENTRIES[int(rng.integers(0, 3))], "advance": advance, "sync": True, "readers": None})
        steps[-1]["readers"] = readers(True)

    def op_of(kind):
        return (kind, int(rng.integers(0, 1000)))

    def usable(kind):
        if kind in ("set_texture", "update_texture_async") and m.big_image and textured:
            return False
        return m.allowed(kind)

    step([[("delta_on", 1)], [("highlight_set", seed)], [("overlay_set", seed)]][start(seed)["first"]], True)      # (what some readers need, from the start)
    for kind, d in targets:
        if len(steps) >= 30:
            break
        for _ in range(3):                                   # what the operation needs first, in an earlier gap
            if usable(kind) or kind not in _FIXES:
                break
            fix = _FIXES[kind]
            if not m.allowed(fix):
                break
            step([op_of(fix)])
        if kind in ASYNC and not m.allowed(kind):
            step([])
        if not usable(kind):
            continue
        mode = int(rng.integers(0, 3))                       # the rest before it: lights moving, lights still, either
        while (rest.last_class != d if d < 3 else rest.depth < 4 + int(rng.integers(0, 3))) and len(steps) < 39:
            if rest.last_class is not None and rest.last_class > d:
                step([op_of("camera_ulp")])                  # (too deep already: end the rest)
            else:
                step([], (True, False, None)[mode])
        # every kind shares its gap with another family at two of the four depths and stands alone at the other two (so that a
        # lighting-side change also meets a resting frame that nothing else ends).  Alone, a cubemap is replaced by one of the same
        # size with other texels: no uniform moves, only the cubemap's generation tells.
        paired = (d + OP_KINDS.index(kind)) % 2 == 0
        ops = [op_of(kind)]
        if kind == "set_cubemap" and not paired:
            ops = [(kind, 1 + 3 * int(rng.integers(0, 300)))]
        if kind in ("set_texture", "update_texture_async"):
            textured += 1
        if paired and kind not in ("object_add", "scene_clear", "resize"):
            for c in rng.permutation(len(_COMPANIONS)):
                ck = _COMPANIONS[c]
                if FAMILY[ck] != FAMILY[kind] and usable(ck) and not (ck in ("set_texture",) and m.big_image):
                    ops.insert(int(rng.integers(0, 2)), op_of(ck))
                    break
        elif paired:
            ops.append(op_of(("camera_jump", "sun_move")[int(rng.integers(0, 2))]))
        step(ops)
    while len(steps) < 24:
        step([], (True, False, None)[int(rng.integers(0, 3))])
    # a stretch with no host synchronisation: operations go on, only the device-form readers are left
    if start(seed)["stretch"]:
        n = int(rng.integers(4, 13))
        with_ops = [i for i in range(2, len(steps) - n) if any(s["ops"] for s in steps[i:i + n])]
        a = with_ops[int(rng.integers(0, len(with_ops)))]
        replay, rr = Model(seed), Rest()
        for i, s in enumerate(steps):
            for op in s["ops"]:
                replay.apply(op)
            rr.gap([k for k, _ in s["ops"]], s["advance"]); rr.frame(); replay.frame_done()
            if a <= i < a + n:
                s["sync"] = False
                s["readers"] = [(k, j) for k, j in ((kk, i * 7 + q) for q, kk in enumerate(DEVICE_READERS)) if replay.reader_allowed(k)][:2]
    return steps


# ------------------------------------------------------------------------------------------------ playing a script

class Hooks:
    """What a player of steps does at each point; the default does nothing.  frame(i, step, model, rest, oracle): after frame i was
    enqueued on both sides, `rest` = Rest.frame()'s answer; reader(i, step, reader, model, oracle); end(model)."""

    def dev(self, a, row):
        raise NotImplementedError

    def frame(self, i, step, m, rest, o):
        pass

    def reader(self, i, step, reader, m, o):
        pass

    def end(self, m):
        pass


class OracleOf:
    """The oracle for the model's current state, built anew when the scene's version moved; a frame of the same version, camera, sun and
    stage re-runs its lighting pass only (zo_render's pass mask)."""

    def __init__(self, lib):
        self.lib, self.o, self.key, self.version = lib, None, None, None

    def frame(self, m):
        if self.o is None or self.version != m.version:
            if self.o is not None:
                self.o.close()
            self.o = self.lib.Oracle(m.W, m.H, m.SD)
            m.populate(self.o, oracle=True)
            self.version, self.key = m.version, None
        self.o.set_shading(m.forward)
        key = (m.version, m.sun, m.roll_stage, m.cam, m.ulps, m.forward)
        m.uniforms(self.o)
        self.o.render(m.view, 7 if key != self.key else 4)
        self.key = key
        return self.o


def run(steps, upto=None, seed=0, oracle_lib=None, renderer=None, hooks=None):
    """Plays steps[:upto] of the session of `seed` (its model's starting state and flavour) on the oracle and, when given, on a renderer
    (created by the caller at the model's extent: see Model(seed)); -> the model.  A failing session is cut down by passing fewer steps."""
    hooks = hooks or Hooks()
    m, rest = Model(seed), Rest()
    chk = OracleOf(oracle_lib) if oracle_lib is not None else None
    g = renderer
    if g is not None:
        m.populate(g)
        g.set_id_capture(m.capture)
    for i, s in enumerate(steps[:upto]):
        for op in s["ops"]:
            m.apply(op, g, hooks.dev)
        rest.gap([k for k, _ in s["ops"]], s["advance"])
        if s["advance"]:
            m.tick += 1
        if g is not None:
            m.uniforms(g)
            if s["entry"] == "staged":
                g.render_shadow(); g.render_gbuffer(); g.render_lighting()
            elif s["entry"] == "geometry":
                g.render_geometry(); g.render_lighting()
            else:
                g.render()
            if s["sync"]:
                g.finish()
        o = chk.frame(m) if chk else None
        m.frame_done()
        hooks.frame(i, s, m, rest.frame(), o)
        for rd in s["readers"]:
            hooks.reader(i, s, rd, m, o)
    hooks.end(m)
    return m
