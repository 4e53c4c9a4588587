"""The scenes the independent statements are evaluated on (tests/independent_eval.py, tests/independent_geometry.py).  TEST INFRASTRUCTURE.

`Scene` collects draws for the oracle, the HIP renderer (same method names) and the evaluators; `SCENES` are the three named and ten
random scenes of tests/test_oracle_independent.py; `EDGE_SCENES` are the geometry edges of tests/test_oracle_geometry.py and
tests/test_gpu_independent.py (each returns a `Case`).
"""
import collections
import math

import numpy as np

from zeldaengine_amd import abi, scenes

DEFAULT_TEXELS = [(127, 127, 127, 255), (0, 0, 0, 255), (255, 255, 255, 255), (127, 127, 255, 255), (255, 255, 255, 255), (0, 0, 0, 255),
                  (255, 255, 255, 255)]                      # default_{grey,black,white,normal,white,black,white}.png, ZE:4951-4978
FACES = [(200, 60, 40, 255), (40, 180, 70, 255), (50, 80, 210, 255), (220, 200, 60, 255), (150, 150, 160, 255), (30, 30, 35, 255)]


def _const(rgba, n=2):
    return np.tile(np.array(rgba, dtype=np.uint8), (n, n, 1))


class Scene:
    """Collects draws for both the oracle and the independent evaluator (engine draw order: non-instanced first, ZE:3445-3476)."""

    def __init__(self, cube=None):
        self.items = []
        self.cube = cube                 # six (d, d, 4) uint8 faces, or None: FACES, one colour per 4 x 4 face

    def add(self, mesh, texels=None, instances=None, images=None):
        """texels: 7 constant RGBA8 slots (None: the engine's defaults); images: 7 entries, each None (the engine's default texel) or an
        (h, w, 4) uint8 image, given to the renderer as it is (the statement samples the images that are not constant)"""
        given = sampled = None
        if images is not None:
            given = [None if im is None else np.ascontiguousarray(im, np.uint8) for im in images]
            texels = [DEFAULT_TEXELS[i] if im is None else tuple(int(x) for x in im[0, 0]) for i, im in enumerate(given)]
            sampled = [None if im is None or (im == im[0, 0]).all() else im for im in given]
        self.items.append({"verts": mesh[0], "idx": mesh[1], "texel": list(texels or DEFAULT_TEXELS), "instances": instances,
                           "images": sampled, "given": given})

    def load(self, o):
        o.set_cubemap(self.cube if self.cube is not None else [_const(c, 4) for c in FACES])
        self._keep = []
        for it in self.items:
            mat = None
            if it["given"] is not None:
                mat, k = abi.make_material(it["given"])
                self._keep.append(k)
            elif it["texel"] != DEFAULT_TEXELS:
                mat, k = abi.make_material([_const(t) for t in it["texel"]])
                self._keep.append(k)
            o.object_add(o.mesh_create(it["verts"], it["idx"]), mat, it["instances"])

    def cube_statement(self):
        """what lighting() takes for this scene's cubemap: the face colours, or the chain of a sampled cubemap"""
        import independent_sampler as isamp
        return FACES if self.cube is None else isamp.cube_chain(self.cube)

    def draws(self):
        out, base = [], 0
        for instanced in (False, True):
            for it in self.items:
                if (it["instances"] is not None) != instanced:
                    continue
                d = dict(it)
                d["prim_base"] = base
                base += (len(it["idx"]) // 3) * (1 if it["instances"] is None else len(it["instances"]))
                out.append(d)
        return out


def _lights(n_dir, n_point):
    w = scenes.sample_world()
    d, _, s = scenes.lights_from_world(w)
    w["PointLights"] = scenes.sample_point_lights(n_point)
    _, p, _ = scenes.lights_from_world(w)
    for l in p:
        l["Direction"][3] = 6.0           # a radius that reaches the geometry
    return d[:n_dir], p, s


def scene_mixed():
    s = Scene()
    s.add(scenes.grid_plane(14.0, 3, 0.0))
    s.add(scenes.box((0.9, 0.6, 0.5), (1.2, -0.8, 0.5)), [(200, 40, 30, 255), (255, 255, 255, 255), (90, 90, 90, 255), (127, 127, 255, 255),
                                                            (180, 180, 180, 255), (0, 20, 40, 255), (255, 255, 255, 255)])
    s.add(scenes.uv_sphere(12, 6, 0.6), None, scenes.generate_instances(12, 1.0, 4.5, 0.5, 1.2, seed=3))
    return s, abi.make_camera((5.0, 4.0, 3.5), (0.0, 0.0, 0.4)), _lights(1, 4), 0.0


def scene_single_sphere_no_sun():
    """config 2's shape: no directional light -> lookAt(0, 0) = NaN shadow matrices -> every PCF tap returns 1"""
    s = Scene()
    s.add(scenes.uv_sphere(16, 8, 1.0))
    return s, abi.make_camera((1.9, 1.7, 1.3), (0.0, 0.0, 0.0)), _lights(0, 1), 0.0


def scene_rolled_and_clipped():
    """a rotated stage (model != identity), metallic / rough materials, instanced boxes, the ground crossing the near plane"""
    s = Scene()
    s.add(scenes.grid_plane(40.0, 2, 0.0), [(90, 140, 60, 255), (0, 0, 0, 255), (200, 200, 200, 255), (127, 127, 255, 255), (255, 255, 255, 255),
                                             (0, 0, 0, 255), (255, 255, 255, 255)])
    s.add(scenes.box((0.4, 0.4, 0.9), (0, 0, 0.9)), [(220, 220, 230, 255), (230, 230, 230, 255), (60, 60, 60, 255), (140, 120, 250, 255),
                                                      (255, 255, 255, 255), (10, 0, 0, 255), (255, 255, 255, 255)],
          scenes.generate_instances(9, 1.5, 5.0, 0.6, 1.4, seed=21))
    s.add(scenes.uv_sphere(10, 5, 0.8), None, scenes.generate_instances(5, 1.0, 3.0, 0.5, 1.0, seed=4))
    return s, abi.make_camera((3.0, -4.0, 1.2), (0.0, 0.0, 0.6), fov=60.0), _lights(1, 16), 0.35


def scene_random(seed):
    """seeded mixtures: 2-5 draws of plane / box / sphere with random constant materials (metallic, rough, emissive, masked, odd normal
    texels), with and without instances, 0-1 directional and 0-24 point lights, the camera anywhere around, the stage rolled"""
    rng = np.random.default_rng(7000 + seed)
    s = Scene()

    def texels():
        if rng.random() < 0.3:
            return None
        t = [tuple(int(x) for x in rng.integers(0, 256, 3)) + (255,) for _ in range(7)]
        t[3] = (int(rng.integers(100, 156)), int(rng.integers(100, 156)), int(rng.integers(200, 256)), 255)      # a plausible normal texel
        t[6] = (int(rng.choice([255, 255, 255, 0, 128])), 0, 0, 255)                                              # the lighting mask
        return t
    s.add(scenes.grid_plane(float(rng.choice([10.0, 24.0, 60.0])), int(rng.integers(2, 5)), 0.0), texels())
    for _ in range(int(rng.integers(1, 5))):
        kind = int(rng.integers(0, 3))
        mesh = [scenes.uv_sphere(12, 6, 0.6), scenes.uv_sphere(16, 8, 0.9), scenes.box((0.7, 0.5, 0.6), (0.0, 0.0, 0.6))][kind]
        inst = scenes.generate_instances(int(rng.integers(2, 20)), 0.8, float(rng.uniform(3.0, 9.0)), 0.4, 1.3, seed=int(rng.integers(1, 1 << 30))) if rng.random() < 0.7 else None
        s.add(mesh, texels(), inst)
    a, rad = rng.uniform(0, 2 * math.pi), float(rng.choice([3.5, 6.0, 11.0]))
    cam = abi.make_camera((rad * math.cos(a), rad * math.sin(a), float(rng.choice([0.6, 2.0, 5.0]))), (float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)), 0.4),
                          fov=float(rng.choice([40.0, 55.0, 70.0])))
    return s, cam, _lights(int(rng.integers(0, 2)), int(rng.choice([0, 1, 3, 8, 24]))), float(rng.uniform(0.0, 1.0))


SCENES = {"mixed": scene_mixed, "single_sphere_no_sun": scene_single_sphere_no_sun, "rolled_and_clipped": scene_rolled_and_clipped}
for _k in range(10):
    SCENES["random_%02d" % _k] = (lambda k: (lambda: scene_random(k)))(_k)


# ---------------------------------------------------------------------------------------------------------------- geometry edge cases

Case = collections.namedtuple("Case", "scene cam lights roll_stage roll_light W H SD")


def case(name, W=192, H=128, SD=256):
    """One of SCENES (roll_light 0) or EDGE_SCENES as a Case; the edge scenes carry their own size."""
    if name in EDGE_SCENES:
        return EDGE_SCENES[name]()
    s, cam, lights, roll = SCENES[name]()
    return Case(s, cam, lights, roll, 0.0, W, H, SD)


def _sun_at(lights, elevation, azimuth=0.0, distance=28.0):
    """the first directional light moved to (elevation, azimuth) at `distance`: its Position is the shadow camera's eye (ZE:4606-4612)"""
    d, p, s = lights
    d = d.copy()
    ce = 0.0 if elevation == math.pi / 2 else math.cos(elevation)          # the zenith exactly: cos(pi / 2) is 6e-17 in float64
    d[0]["Position"][:3] = (distance * ce * math.cos(azimuth), distance * ce * math.sin(azimuth), distance * math.sin(elevation))
    return d, p, s


def _props(s, n_boxes=14, n_spheres=8, seed=5, radius=4.0):
    s.add(scenes.box((0.5, 0.4, 0.6), (0.0, 0.0, 0.6)), None, scenes.generate_instances(n_boxes, 0.8, radius, 0.5, 1.3, seed=seed))
    s.add(scenes.uv_sphere(12, 6, 0.6), None, scenes.generate_instances(n_spheres, 1.0, radius, 0.5, 1.2, seed=seed + 1))


def edge_rolled_stage_and_light():
    """roll_stage and roll_light both nonzero: the stage rolls in both Model matrices, the point-light spiral turns (ZE:4606-4646)"""
    s = Scene()
    s.add(scenes.grid_plane(14.0, 3, 0.0))
    _props(s)
    return Case(s, abi.make_camera((5.0, 4.0, 3.5), (0.0, 0.0, 0.4)), _lights(1, 12), 0.6, 0.8, 192, 128, 256)


def edge_grazing_sun():
    """the sun 0.15 rad above the horizon, a 1024-texel map: long, steep shadow-space slopes (the 7.5 m term dominates)"""
    s = Scene()
    s.add(scenes.grid_plane(20.0, 4, 0.0))
    _props(s, seed=9)
    return Case(s, abi.make_camera((6.0, -3.0, 3.0), (0.0, 0.0, 0.3)), _sun_at(_lights(1, 4), 0.15, 0.4), 0.2, 0.0, 192, 128, 1024)


def edge_sun_at_zenith():
    """the sun straight above the stage: lookAt(eye, 0, up) with up parallel to the view direction -> normalize(cross(f, up)) = 0 / 0"""
    s = Scene()
    s.add(scenes.grid_plane(14.0, 3, 0.0))
    _props(s, seed=13)
    return Case(s, abi.make_camera((5.0, 4.0, 3.5), (0.0, 0.0, 0.4)), _sun_at(_lights(1, 4), math.pi / 2, 0.0, 28.0), 0.0, 0.0, 192, 128, 256)


def _mirrored(inst):
    inst = inst.copy()
    inst["InstancePScale"] *= -1.0
    return inst


def edge_mirrored_instances():
    """negative InstancePScale: the instance transform mirrors, so the winding flips and BACK culling keeps the inner faces"""
    s = Scene()
    s.add(scenes.grid_plane(14.0, 3, 0.0))
    s.add(scenes.box((0.5, 0.4, 0.6), (0.0, 0.0, 0.6)), None, _mirrored(scenes.generate_instances(12, 0.8, 4.0, 0.5, 1.3, seed=17)))
    s.add(scenes.uv_sphere(12, 6, 0.6), None, _mirrored(scenes.generate_instances(6, 1.0, 4.0, 0.5, 1.2, seed=18)))
    s.add(scenes.uv_sphere(12, 6, 0.6), None, scenes.generate_instances(4, 1.0, 4.0, 0.5, 1.2, seed=19))
    return Case(s, abi.make_camera((5.0, 4.0, 3.5), (0.0, 0.0, 0.4)), _lights(1, 4), 0.1, 0.0, 192, 128, 256)


def edge_low_camera():
    """the camera 0.25 above a 30-unit ground plane, znear 0.05, fov 70: triangles cross the near plane and the 4x guard band"""
    s = Scene()
    s.add(scenes.grid_plane(30.0, 12, 0.0))
    _props(s, n_boxes=10, n_spheres=6, seed=23, radius=6.0)
    return Case(s, abi.make_camera((0.4, -0.3, 0.25), (6.0, 4.0, 0.1), fov=70.0, znear=0.05, zfar=80.0), _lights(1, 4), 0.0, 0.0, 192, 128, 256)


def edge_repeated_draw():
    """the same box drawn twice, and the same instanced draw twice: exactly equal depths, so LESS keeps the FIRST draw's primitive"""
    s = Scene()
    s.add(scenes.grid_plane(14.0, 3, 0.0))
    box = scenes.box((0.9, 0.6, 0.5), (1.2, -0.8, 0.5))
    s.add(box)
    s.add(box)
    inst = scenes.generate_instances(10, 1.0, 4.5, 0.5, 1.2, seed=29)
    s.add(scenes.uv_sphere(12, 6, 0.6), None, inst)
    s.add(scenes.uv_sphere(12, 6, 0.6), None, inst)
    return Case(s, abi.make_camera((5.0, 4.0, 3.5), (0.0, 0.0, 0.4)), _lights(1, 4), 0.0, 0.0, 192, 128, 256)


def edge_odd_size():
    """257 x 131 with a 100-texel map: no size is a multiple of the 32-pixel tile or a power of two"""
    s, cam, lights, roll = scene_mixed()
    return Case(s, cam, lights, roll, 0.0, 257, 131, 100)


def _light_mesh(eye, pts, tris):
    """a mesh of points given in the frame of a light at `eye` looking at the origin with up +Z (glm::lookAt, ZE:4610): (a, b, d) ->
    eye + a s + b u + d f, f = normalize(-eye), s = normalize(f x Z), u = s x f"""
    eye = np.asarray(eye, dtype=np.float64)
    f = -eye / np.linalg.norm(eye)
    s = np.cross(f, (0.0, 0.0, 1.0))
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    world = [tuple(eye + a * s + b * u + d * f) for a, b, d in pts]
    return scenes._ingest(world, [(0.0, 0.0, 1.0)] * len(world), [(0.0, 0.0)] * len(world), [tuple((i, 0) for i in t) for t in tris])


def edge_shadow_near_sliver():
    """the light's near plane (zNear 6.0005, the camera's) just beyond the look-at point, which is a vertex of a 30-unit ground plane
    in 24 x 24 cells under a sun 74 degrees high and 6 away: the plane crosses the near plane at 16 degrees, the vertex at the origin
    lies 0.0005 behind it, and the clipper's polygons around it hold three vertices whose triangle is under 1/8 texel high on the
    1024-texel map (tests/test_oracle_geometry.py computes it)"""
    s = Scene()
    s.add(scenes.grid_plane(30.0, 24, 0.0))
    _props(s, n_boxes=8, n_spheres=4, seed=31, radius=3.0)
    return Case(s, abi.make_camera((6.5, -5.0, 4.5), (0.0, 0.0, 0.0), znear=6.0005, zfar=60.0), _sun_at(_lights(1, 4), 1.3, 0.7, 6.0),
                0.0, 0.0, 192, 128, 1024)


def edge_shadow_behind_light():
    """a 160-unit ground plane in 4 x 4 cells under a sun 0.45 rad high at 28: the plane runs on behind the light, where w <= 0, so
    the triangles under the light cross w = 0 and the near plane"""
    s = Scene()
    s.add(scenes.grid_plane(160.0, 4, 0.0))
    _props(s, n_boxes=10, n_spheres=6, seed=37)
    return Case(s, abi.make_camera((5.0, 4.0, 3.5), (0.0, 0.0, 0.4), zfar=120.0), _sun_at(_lights(1, 4), 0.45, 2.2, 28.0), 0.0, 0.0, 192, 128, 512)


SLAB = (63.5, 64.0)       # zNear, zFar: far / (far - near) = 128, so z / w reaches 64 at twice the near distance


def _slab(caster):
    """the camera and the sun at the same eye, 5 from the origin, 85 degrees high, fov 20, zNear 63.5, zFar 64: a 12-unit square held
    in the slab 63.75 along the eye's axis (the origin stays near the eye, so the matrices' translations do not cancel), and `caster`,
    three points in the eye's frame (a, b, depth along the axis)"""
    lights = _sun_at(_lights(1, 4), 1.48, 0.3, 5.0)
    eye = lights[0][0]["Position"][:3]
    grid = [(a, b, 63.75 + 0.02 * a) for b in (-6.0, -2.0, 2.0, 6.0) for a in (-6.0, -2.0, 2.0, 6.0)]
    quads = [(4 * i + j, 4 * i + j + 1, 4 * i + j + 5) for i in range(3) for j in range(3)] + \
            [(4 * i + j, 4 * i + j + 5, 4 * i + j + 4) for i in range(3) for j in range(3)]
    s = Scene()
    s.add(_light_mesh(eye, grid, quads))
    s.add(_light_mesh(eye, caster, [(0, 1, 2)]))
    return Case(s, abi.make_camera(tuple(float(x) for x in eye), (0.0, 0.0, 0.0), fov=20.0, znear=SLAB[0], zfar=SLAB[1]), lights,
                0.0, 0.0, 192, 128, 1024)


def edge_shadow_far_cut():
    """a caster beside the slab's square from 63.6 to 128 along the axis: its far vertex at z / w = 64.5, x / w = 3 (inside the guard
    band), so r from that vertex is 2^6 times the far-clipped polygon's"""
    return _slab([(7.0, -6.0, 63.6), (7.0, 6.0, 63.6), (67.6, 0.0, 128.0)])


def edge_shadow_both_planes():
    """one triangle from 63.2 (in front of the near plane) to 100 (beyond the far plane) beside the slab's square: clipped by both"""
    return _slab([(-7.0, -6.0, 63.2), (-7.0, 6.0, 63.2), (-30.0, 0.0, 100.0)])


EDGE_SCENES = {"rolled_stage_and_light": edge_rolled_stage_and_light, "grazing_sun": edge_grazing_sun, "sun_at_zenith": edge_sun_at_zenith,
               "mirrored_instances": edge_mirrored_instances, "low_camera": edge_low_camera, "repeated_draw": edge_repeated_draw,
               "odd_size": edge_odd_size, "shadow_near_sliver": edge_shadow_near_sliver, "shadow_behind_light": edge_shadow_behind_light,
               "shadow_far_cut": edge_shadow_far_cut, "shadow_both_planes": edge_shadow_both_planes}


# ---------------------------------------------------------------------------------------------------------------- textured scenes
# Sampled materials and a sampled cubemap (tests/test_oracle_textured.py, tests/test_gpu_independent.py): images of noise, smooth
# gradients and a one-texel checker; all seven slots of one power-of-two size (the renderer's packed-material form), mixed sizes with
# non-powers of two, and materials with default and constant slots; a grazing ground plane whose UVs leave [0, 1] (REPEAT, up to 16
# anisotropic taps, deep minification), a magnified close-up, instanced spheres whose silhouettes put helper lanes off the triangle; a
# 32-texel noise cubemap and roughness images spanning 0.01-1, so that reflection lods 0-4 all occur.

def _noise(w, h, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w, 4), dtype=np.uint8)


def _gradient(w, h, lo=3, hi=255, seed=0):
    """smooth: R along x, G along y, B along the diagonal, A opaque - R spans lo..hi (roughness 0.01 .. 1 for lo = 3)"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    fx, fy = (xx + 0.5) / w, (yy + 0.5) / h
    img = np.stack([lo + (hi - lo) * fx, lo + (hi - lo) * fy, lo + (hi - lo) * 0.5 * (fx + fy), np.full_like(fx, 255.0)], axis=-1)
    if seed:
        img[..., :3] = np.roll(img[..., :3], seed, axis=-1)
    return np.round(img).astype(np.uint8)


def _checker(w, h, a=(250, 250, 250, 255), b=(20, 40, 60, 255), period=1):
    yy, xx = np.mgrid[0:h, 0:w]
    odd = ((xx // period + yy // period) & 1).astype(bool)
    return np.where(odd[..., None], np.array(b, np.uint8), np.array(a, np.uint8)).astype(np.uint8)


def _normal_map(w, h, seed):
    """plausible tangent-space normals: x, y around 0, z towards the viewer"""
    img = _noise(w, h, seed, 70, 186)
    img[..., 2] = np.random.default_rng(seed + 1).integers(200, 256, (h, w), dtype=np.uint8)
    img[..., 3] = 255
    return img


def _uv_affine(mesh, scale, offset):
    v, idx = mesh
    v = v.copy()
    v["TexCoord"] = v["TexCoord"] * np.float32(scale) + np.asarray(offset, np.float32)
    return v, idx


def _noise_cube(d=32, seed=61):
    return [_noise(d, d, seed + f) for f in range(6)]


def _packed_material(seed):
    """seven 64 x 64 images: the packed form"""
    return [_noise(64, 64, seed), _gradient(64, 64, 0, 255, 1), _gradient(64, 64), _normal_map(64, 64, seed + 2),
            _checker(64, 64, (255, 255, 255, 255), (90, 90, 90, 255)), _noise(64, 64, seed + 3, 0, 60), _checker(64, 64, (255, 0, 0, 255), (150, 0, 0, 255), 4)]


def _textured_lights():
    return _lights(1, 6)


def tex_packed(W=192, H=128, SD=256):
    """a grazing ground plane (UVs x 6, offset: REPEAT, N up to 16, deep minification) and textured instanced spheres"""
    s = Scene(_noise_cube())
    s.add(_uv_affine(scenes.grid_plane(16.0, 2, 0.0), 8.0, (-2.3, 0.7)), images=_packed_material(71))
    s.add(_uv_affine(scenes.uv_sphere(16, 8, 0.7), 2.0, (0.25, -0.5)), None, scenes.generate_instances(10, 1.0, 5.0, 0.6, 1.2, seed=72),
          images=_packed_material(81))
    return Case(s, abi.make_camera((0.5, -12.0, 1.4), (0.0, 2.0, -0.4), fov=60.0), _textured_lights(), 0.0, 0.0, W, H, SD)


def tex_mixed_sizes(W=192, H=128, SD=256):
    """per-slot sizes 48 x 20, 33 x 7, 1 x 16, 64 x 64, 16 x 32, 128 x 4, 8 x 8: a magnified close-up of a box, a sphere and the ground"""
    mat = [_noise(48, 20, 91), _gradient(33, 7, 0, 255, 2), _gradient(1, 16, seed=2), _normal_map(64, 64, 93), _checker(16, 32, period=2),
           _noise(128, 4, 94, 0, 80), _checker(8, 8, (255, 0, 0, 255), (120, 0, 0, 255))]
    s = Scene(_noise_cube(32, 95))
    s.add(_uv_affine(scenes.grid_plane(10.0, 8, 0.0), 3.0, (0.1, 0.3)), images=mat)
    s.add(scenes.box((0.6, 0.6, 0.6), (0.0, 0.0, 0.6)), images=mat)
    s.add(_uv_affine(scenes.uv_sphere(16, 8, 0.5), 1.0, (0.0, 0.0)), None, scenes.generate_instances(3, 1.0, 2.5, 0.8, 1.0, seed=96), images=mat)
    return Case(s, abi.make_camera((1.25, -1.55, 1.5), (0.0, 0.0, 0.7), fov=60.0), _textured_lights(), 0.0, 0.0, W, H, SD)


def tex_partial(W=192, H=128, SD=256):
    """default (None) and constant slots next to sampled ones: the renderer's per-slot path"""
    mat = [_checker(32, 32, (230, 200, 40, 255), (40, 60, 200, 255)), None, _gradient(16, 16, 3, 255, 0), None, _const((200, 0, 0, 255), 4),
           _noise(8, 8, 97, 0, 50), None]
    mat2 = [None, _const((255, 0, 0, 255), 8), _noise(32, 16, 98, 3, 256), _normal_map(16, 16, 99), None, None, _const((255, 0, 0, 255), 2)]
    s = Scene(_noise_cube(32, 101))
    s.add(_uv_affine(scenes.grid_plane(16.0, 8, 0.0), 4.0, (-0.6, -1.4)), images=mat)
    s.add(_uv_affine(scenes.uv_sphere(16, 8, 0.7), 3.0, (0.0, 0.0)), None, scenes.generate_instances(14, 1.0, 4.5, 0.5, 1.3, seed=102), images=mat2)
    return Case(s, abi.make_camera((5.5, -4.0, 3.0), (0.0, 0.0, 0.3), fov=55.0), _textured_lights(), 0.0, 0.0, W, H, SD)


def tex_clipped(W=192, H=128, SD=256):
    """a coarse 40-unit ground plane (two triangles a side) under a camera 0.3 above it, znear 0.05: every visible ground triangle
    crosses the near plane, so its sampled slots are held to the clipped polygon's budget, not excused"""
    s = Scene(_noise_cube(32, 103))
    s.add(_uv_affine(scenes.grid_plane(40.0, 2, 0.0), 10.0, (0.3, -0.2)), images=_packed_material(104))
    s.add(_uv_affine(scenes.uv_sphere(16, 8, 0.7), 2.0, (0.0, 0.0)), None, scenes.generate_instances(6, 1.0, 4.0, 0.6, 1.2, seed=105),
          images=_packed_material(106))
    return Case(s, abi.make_camera((0.4, -0.3, 0.3), (6.0, 4.0, 0.0), fov=70.0, znear=0.05, zfar=80.0), _textured_lights(), 0.0, 0.0, W, H, SD)


TEXTURED_SCENES = {"tex_clipped": tex_clipped, "tex_packed": tex_packed, "tex_mixed_sizes": tex_mixed_sizes, "tex_partial": tex_partial,
                   "tex_packed_257x131": lambda: tex_packed(257, 131, 100), "tex_mixed_sizes_33x17": lambda: tex_mixed_sizes(33, 17, 64)}


# ---------------------------------------------------------------------------------------------------------------- skydome and background
# The skydome and background passes (tests/test_oracle_sky.py, tests/test_gpu_independent.py): the dome of scenes.sky_dome() and a coarse
# 16 x 8 one whose visible triangles straddle the camera's plane (the near plane cuts them), a zFar that cuts the dome, a rolled stage,
# a camera looking near the pole (the longitude lines converge: large, anisotropic derivatives, N clamps at 16), noise and NPOT sky
# images (a smooth gradient would not tell one lod from another), background images magnified on one axis and minified on the other.
# The sizes: 192 x 128, 257 x 131, 33 x 17, 64 x 64 (pixel centres on the diagonal of the lighting quad, view 6) and 200 x 120 with
# unequal editor bars (view 9's mosaic, ViewportInfo.zw = 37, 21).

SkyCase = collections.namedtuple("SkyCase", "case sky sky_image background bars")


def _sky_case(W, H, SD=128, cam=None, roll=0.0, dome=None, sky_image=None, background=None, bars=(0.0, 0.0), no_dome=False):
    s, cam0, lights, _ = scene_mixed()
    return SkyCase(Case(s, cam or cam0, lights, roll, 0.0, W, H, SD), None if no_dome else dome if dome is not None else scenes.sky_dome(),
                   sky_image if sky_image is not None else _noise(256, 128, 111), background, bars)


def sky_dome_noise(W=192, H=128):
    """the engine's dome stand-in with a noise sky; zFar 26 cuts it where it is farthest (the background shows there); the background
    minified in x, magnified in y"""
    return _sky_case(W, H, cam=abi.make_camera((6.0, 5.0, 2.0), (0.0, 0.0, 1.5), zfar=26.0), background=_noise(410, 40, 112))


def sky_coarse_clipped(W=192, H=128):
    """a 16 x 8 dome (8-unit triangles), the camera 2.5 from its wall looking along it: the triangles around the camera straddle its
    plane, and the near plane cuts half of what is visible"""
    return _sky_case(W, H, cam=abi.make_camera((18.0, 0.0, 3.0), (18.0, 10.0, 5.0), fov=90.0, znear=0.1, zfar=100.0),
                     dome=scenes.sky_dome(20.48, 16, 8), sky_image=_noise(128, 64, 113), background=_noise(40, 300, 114))


def sky_rolled_npot(W=192, H=128):
    """the stage rolled by 0.6 (the dome's Model), an NPOT 200 x 75 sky, no background"""
    return _sky_case(W, H, cam=abi.make_camera((5.0, 4.0, 3.5), (0.0, 0.0, 0.4), zfar=100.0), roll=0.6, sky_image=_noise(200, 75, 115))


def sky_pole(W=192, H=128):
    """a camera looking almost straight up at the pole: the longitude lines converge, derivatives large and anisotropic; with a wide
    1024 x 48 sky (u spans 1024 texels, v 48) Pmax / Pmin reaches 57 and exceeds 16 on ~9 % of the dome's pixels, where N clamps"""
    return _sky_case(W, H, cam=abi.make_camera((0.5, 0.3, 2.0), (0.52, 0.35, 12.0), fov=70.0, zfar=100.0), sky_image=_noise(1024, 48, 116),
                     background=_noise(64, 64, 117))


def background_only(W=192, H=128):
    """no dome: the background behind the scene on every empty pixel, its right and bottom columns included (REPEAT wraps the
    bilinear footprint there); 410 x 40 texels: minified in x, magnified in y"""
    return _sky_case(W, H, background=_noise(410, 40, 118), no_dome=True)


SKY_SCENES = {"background_only": background_only, "sky_dome_noise": sky_dome_noise, "sky_coarse_clipped": sky_coarse_clipped, "sky_rolled_npot": sky_rolled_npot, "sky_pole": sky_pole,
              "sky_dome_257x131": lambda: sky_dome_noise(257, 131), "sky_coarse_33x17": lambda: sky_coarse_clipped(33, 17),
              "sky_rolled_64x64": lambda: sky_rolled_npot(64, 64),
              "sky_bars_200x120": lambda: sky_dome_noise(200, 120)._replace(bars=(37.0, 21.0))}
