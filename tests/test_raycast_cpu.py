"""Casting rays without a GPU: the host statement of the rule (zr_ray_triangles, csrc/zr_raycast.h) against the independent float64
statement (tests/raycast_reference.py), its watertightness, its details, the stand-alone program under the sanitizers
(tests/raycast_check.cpp) and the ABI of the new entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import raycast_cases as rcc
import raycast_reference as rr
from zeldaengine_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zeldaengine_amd", "csrc")
NAMES = ("zr_raycast", "zr_raycast_async", "zr_camera_ray", "zr_ray_triangles")
MISS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    """tests/raycast_check.cpp, which includes csrc/zr_raycast.h alone, under the address and undefined-behaviour sanitizers where this
    machine links them for a stand-alone program (as tests/test_overlay_cpu.py does with its own)"""
    tmp = tmp_path_factory.mktemp("raycast_check")
    flags = ["-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    hello = tmp / "hello.cpp"
    hello.write_text("int main() { return 0; }\n")
    if not (subprocess.call(["g++"] + sanitize + [str(hello), "-o", str(tmp / "hello")], stderr=subprocess.DEVNULL) == 0 and
            subprocess.call([str(tmp / "hello")]) == 0):
        sanitize = []
    exe = tmp / "raycast_check"
    subprocess.check_call(["g++"] + flags + sanitize + ["-I", CSRC, os.path.join(ROOT, "tests", "raycast_check.cpp"), "-o", str(exe)])
    return str(exe), tmp


def _one(o, d, tris, flags=0, t_min=0.0, t_max=np.inf):
    return engine.ray_triangles(abi.make_rays([o], [d], t_min, t_max), np.asarray(tris, dtype=np.float32), flags)[0]


def _is_miss(h, flags=0):
    return (h["object"], h["instance"], h["triangle"], h["flags"]) == (MISS, MISS, MISS, flags) and not any(
        (h["t"], h["u"], h["v"], h["reserved"], h["reserved2"])) and not h["normal"].any()


# ---- the ABI

def test_library_exports_the_ray_cast_entry_points():
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    L = engine.lib()
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name + " is not declared"
        assert hasattr(L, name), name + " is not exported"
    for flag, value in (("ZR_RAY_HIT", 1), ("ZR_RAY_HIT_BACK", 2), ("ZR_RAY_INVALID", 4), ("ZR_RAY_CULL_BACK", 1), ("ZR_RAY_ANY_HIT", 2), ("ZR_RAY_NO_BOUNDS", 4)):
        assert re.search(r"#define %s\s+%du\b" % (flag, value), hdr), flag
    assert (abi.RAY_HIT_FLAG, abi.RAY_HIT_BACK, abi.RAY_INVALID, abi.RAY_CULL_BACK, abi.RAY_ANY_HIT, abi.RAY_NO_BOUNDS) == (1, 2, 4, 1, 2, 4)
    assert "#define ZR_ABI_VERSION 7u" in hdr and abi.ABI_VERSION == 7 == L.zr_abi_version()      # additive: no bump


def test_ray_structs_are_32_and_48_bytes_in_c_ctypes_and_numpy(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "zelda_render.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu", sizeof(zr_ray), '
                   'offsetof(zr_ray, t_min), offsetof(zr_ray, dir), offsetof(zr_ray, t_max), sizeof(zr_ray_hit), offsetof(zr_ray_hit, flags), '
                   'offsetof(zr_ray_hit, t), offsetof(zr_ray_hit, normal));return 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    R, H = abi.Ray, abi.RayHit
    assert got == [32, 12, 16, 28, 48, 12, 16, 32] == [C.sizeof(R), R.t_min.offset, R.dir.offset, R.t_max.offset, C.sizeof(H), H.flags.offset, H.t.offset, H.normal.offset]
    D, E = abi.RAY, abi.RAY_RECORD
    assert [D.itemsize, D.fields["t_min"][1], D.fields["dir"][1], D.fields["t_max"][1], E.itemsize, E.fields["flags"][1], E.fields["t"][1], E.fields["normal"][1]] == got


def test_rule_header_is_plain_cpp_and_names_no_hip_header():
    text = open(os.path.join(CSRC, "zr_raycast.h")).read()
    assert "hip/" not in text and "zr_dev.h" not in text and "zr_types.h" not in text
    assert "zr_raycast.hip" in open(os.path.join(ROOT, "zeldaengine_amd", "build.py")).read()


# ---- against the float64 statement

def test_ray_triangles_against_the_float64_reference():
    """8 spheres of 960 triangles, 1 500 rays at triangle interiors (weights >= 0.1, incidence cosine >= 0.2): the same triangle on every
    unambiguous ray, t, u, v and the normal within the derived bounds, at most 1 % of the rays excused.
    (Measured here: see DESIGN.md section 6 for the largest error / bound ratio.)"""
    draws = rcc.draws_of(rcc.sphere_cluster())
    tris64, err, _ = rr.world_triangles(draws, np.eye(4))
    tris32 = rcc.world_f32(draws, np.eye(4))
    assert tris32.shape == (7680, 3, 3)
    rays = rcc.rays_at_triangles(np.random.default_rng(11), tris64, 1500)
    hits = engine.ray_triangles(rays, tris32)
    groups = rr.groups_of(tris64, [960] * 8)
    ref = rr.cast(rays["origin"], rays["dir"], rays["t_min"], rays["t_max"], tris64, err, groups=groups)
    n_amb, worst, bad = rr.compare(ref, hits)
    print("zr_ray_triangles vs float64: %d of %d rays ambiguous, %d hits, largest error / bound ratio %.4f" % (n_amb, len(rays), int((ref["prim"] >= 0).sum()), worst))
    assert not bad, bad[:5]
    assert n_amb <= len(rays) // 100
    assert int((ref["prim"] >= 0).sum()) >= 1400           # (the rays were aimed at triangles)
    # ... and with BACK hits culled: the same answers (every ray was aimed at a front), ZR_RAY_ANY_HIT says whether there is one
    culled = engine.ray_triangles(rays, tris32, abi.RAY_CULL_BACK)
    refc = rr.cast(rays["origin"], rays["dir"], rays["t_min"], rays["t_max"], tris64, err, cull_back=True, groups=groups)
    n_amb, _, bad = rr.compare(refc, culled)
    assert not bad and n_amb <= len(rays) // 100
    anyh = engine.ray_triangles(rays, tris32, abi.RAY_ANY_HIT)
    assert np.array_equal(anyh["flags"] & 1, hits["flags"] & 1) and (anyh["object"] == MISS).all() and not anyh["t"].any()


def test_reference_flags_what_it_cannot_decide():
    """the verdict itself: a ray at an edge, at a second surface a hair behind, at a range bound - ambiguous; a clean one - not"""
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, -1e-7], [1, 0, -1e-7], [0, 1, -1e-7]]], dtype=np.float64)
    def amb(o, d, tris, lo=0.0, hi=np.inf):
        return bool(rr.cast([o], [d], lo, hi, tris)["ambiguous"][0])
    assert not amb((0.25, 0.25, 1), (0, 0, -1), tri[:1])
    assert amb((0.5, 0.0, 1), (0, 0, -1), tri[:1])                       # on an edge
    assert amb((0.25, 0.25, 1), (0, 0, -1), tri)                         # a second surface within the tolerance
    assert amb((0.25, 0.25, 1), (0, 0, -1), tri[:1], 0.0, 1.0)           # t on the range bound
    assert amb((0.5 + 1e-9, 0.5, 1), (0, 0, -1), tri[:1])                # a miss by less than the tolerance
    assert not amb((2.0, 2.0, 1), (0, 0, -1), tri[:1])                   # a clean miss
    r = rr.cast([(0.25, 0.25, 1)], [(0, 0, -1)], 0.0, np.inf, tri[:1])
    assert r["prim"][0] == 0 and not r["back"][0] and abs(r["t"][0] - 1.0) < 1e-15 and abs(r["u"][0] - 0.25) < 1e-15
    assert rr.cast([(0.25, 0.25, -1)], [(0, 0, 1)], 0.0, np.inf, tri[:1])["back"][0]


def test_camera_rays_of_the_reference_meet_its_own_raster():
    """what tests/test_gpu_raycast.py relies on, by the float64 statements alone: on the camera scene, a pixel whose 3 x 3 neighbourhood
    in the rasterised winner plane holds one primitive is hit by the camera's ray through its centre in that primitive, in front, with
    t in (0, 1); where the neighbourhood is empty the ray misses; the set is non-empty - at least a quarter of the covered pixels"""
    import independent_geometry as ig
    from independent_scenes import _lights
    scene, cam = rcc.camera_scene(), rcc.camera_of_scene()
    draws = rcc.draws_of(scene)
    fu = ig.frame_uniforms(cam, *_lights(1, 2)[:2], rcc.W, rcc.H)["cam"]
    st = ig.raster(draws, fu, rcc.W, rcc.H)
    prim = st["prim"].astype(np.int64)
    prim[prim == MISS] = -1
    solid = np.zeros(prim.shape, dtype=bool)
    solid[1:-1, 1:-1] = np.all([prim[1 + dy:prim.shape[0] - 1 + dy, 1 + dx:prim.shape[1] - 1 + dx] == prim[1:-1, 1:-1] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    amb = st["ambiguous"]
    near_amb = np.zeros(prim.shape, dtype=bool)
    near_amb[1:-1, 1:-1] = np.any([amb[1 + dy:prim.shape[0] - 1 + dy, 1 + dx:prim.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    solid &= ~near_amb
    assert (solid & (prim >= 0)).sum() >= (prim >= 0).sum() // 4 and (solid & (prim < 0)).sum() > 0
    ys, xs = np.nonzero(solid)
    inv = np.linalg.inv(fu["Proj"] @ fu["View"])
    ndc = np.stack([(xs + 0.5) / (rcc.W / 2) - 1.0, (ys + 0.5) / (rcc.H / 2) - 1.0], axis=1)
    ends = []
    for z in (0.0, 1.0):
        p = np.concatenate([ndc, np.full((len(xs), 1), z), np.ones((len(xs), 1))], axis=1) @ inv.T
        ends.append(p[:, :3] / p[:, 3:])
    tris64, err, _ = rr.world_triangles(draws, fu["Model"])
    ref = rr.cast(ends[0], ends[1] - ends[0], 0.0, 1.0, tris64, err)
    want = prim[ys, xs]
    assert np.array_equal(ref["prim"], want), "%d of %d camera rays name another primitive than the raster" % (int((ref["prim"] != want).sum()), len(want))
    hit = want >= 0
    assert not ref["back"][hit].any() and (ref["t"][hit] > 0).all() and (ref["t"][hit] < 1).all() and not ref["ambiguous"].any()


# ---- watertightness

def test_no_ray_slips_through_a_shared_edge_or_vertex():
    tris, rays, tgt = rcc.dyadic_grid_rays(400)
    hits = engine.ray_triangles(rays, tris)
    assert (hits["flags"] == 1).sum() + (hits["flags"] == 3).sum() == 400, "%d rays leaked" % int((hits["flags"] & 1 == 0).sum())
    for h, (x, y) in zip(hits, tgt):
        assert rcc.holds(tris[h["triangle"]], x, y) and abs(float(h["t"]) - 1.0) <= 8 * 2.0 ** -24
    # where both sharers accept at one t, the lower id: the same rays against the triangles in reverse order name the same triangles
    rev = engine.ray_triangles(rays, tris[::-1].copy())
    same_t = rev["t"] == hits["t"]
    assert (hits["triangle"][same_t].astype(np.int64) <= 127 - rev["triangle"][same_t].astype(np.int64)).all()
    for h, g, (x, y) in zip(hits, rev, tgt):
        assert rcc.holds(tris[::-1][g["triangle"]], x, y)


def test_on_a_shared_edge_the_least_id_wins_where_the_shear_is_exact():
    """the same grid with rays whose shear is exact (the direction's largest component a power of two, the others divisible by it):
    the target lies on the edge for the rule itself, every sharer accepts at t = 1, and the hit is the sharer with the least id -
    whatever order the triangles are visited in"""
    tris, rays, tgt = rcc.dyadic_grid_rays(400, seed=5, exact_shear=True)
    hits = engine.ray_triangles(rays, tris)
    rev = engine.ray_triangles(rays, tris[::-1].copy())
    shared = 0
    for h, g, (x, y) in zip(hits, rev, tgt):
        sharers = [k for k in range(128) if rcc.holds(tris[k], x, y)]
        shared += len(sharers) > 1
        assert h["flags"] & 1 and h["t"] == 1.0 and h["triangle"] == sharers[0], (x, y, h, sharers)
        assert g["flags"] & 1 and g["t"] == 1.0 and 127 - int(g["triangle"]) == sharers[-1], (x, y, g, sharers)
    assert shared == 400


# ---- the rule's details, one small case each

ONE = [[[0, 0, 0], [1, 0, 0], [0, 1, 0]]]


def test_tie_goes_to_the_least_primitive_id():
    h = _one((0.25, 0.25, 2), (0, 0, -1), ONE * 3)
    assert h["triangle"] == 0 and h["flags"] == 1 and h["t"] == 2.0


def test_range_excludes_the_nearest_and_selects_the_next():
    stack = [[[0, 0, 1], [1, 0, 1], [0, 1, 1]], ONE[0]]
    assert _one((0.25, 0.25, 2), (0, 0, -1), stack)["triangle"] == 0
    h = _one((0.25, 0.25, 2), (0, 0, -1), stack, t_min=1.5, t_max=4.0)
    assert h["triangle"] == 1 and h["t"] == 2.0
    assert _is_miss(_one((0.25, 0.25, 2), (0, 0, -1), stack, t_max=0.5))
    assert _one((0.25, 0.25, 2), (0, 0, -1), stack, t_min=1.0, t_max=1.0)["triangle"] == 0       # inclusive


def test_cull_back_and_the_flag_under_a_mirrored_triangle():
    front = _one((0.25, 0.25, 2), (0, 0, -1), ONE)
    back = _one((0.25, 0.25, -2), (0, 0, 1), ONE)
    assert front["flags"] == 1 and back["flags"] == 3 and list(front["normal"]) == [0, 0, 1] == list(back["normal"])
    assert _is_miss(_one((0.25, 0.25, -2), (0, 0, 1), ONE, abi.RAY_CULL_BACK)) and _one((0.25, 0.25, 2), (0, 0, -1), ONE, abi.RAY_CULL_BACK)["flags"] == 1
    mirrored = [[[0, 0, 0], [-1, 0, 0], [0, 1, 0]]]
    assert _one((-0.25, 0.25, 2), (0, 0, -1), mirrored)["flags"] == 3 and _one((-0.25, 0.25, -2), (0, 0, 1), mirrored)["flags"] == 1
    # FRONT is the side the camera pass draws: a float64 d . ((B - A) x (C - A)) < 0
    rng = np.random.default_rng(5)
    for _ in range(50):
        t = rng.uniform(-1, 1, (3, 3)).astype(np.float32)
        p = t.astype(np.float64).mean(axis=0)
        o = (p + rng.uniform(-2, 2, 3)).astype(np.float32)
        d = (p - o).astype(np.float32)
        h = _one(o, d, [t])
        n = np.cross(t[1].astype(np.float64) - t[0], t[2].astype(np.float64) - t[0])
        assert h["flags"] & 1 and bool(h["flags"] & 2) == bool(np.dot(d.astype(np.float64), n) > 0)


def test_an_edge_on_triangle_misses():
    assert _is_miss(_one((0.25, 0, 2), (0, 0, -1), [[[0, 0, 0], [1, 0, 0], [0, 0, 1]]]))


@pytest.mark.parametrize("o,d,lo,hi", [((0, 0, 1), (0, 0, 0), 0.0, 1.0), ((np.nan, 0, 1), (0, 0, -1), 0.0, 1.0), ((0, 0, 1), (0, np.inf, -1), 0.0, 1.0),
                                       ((0, 0, np.inf), (0, 0, -1), 0.0, 1.0), ((0.25, 0.25, 1), (0, 0, -1), np.nan, 1.0), ((0.25, 0.25, 1), (0, 0, -1), 0.0, np.nan),
                                       ((0.25, 0.25, 1), (0, 0, -1), 2.0, 1.0)], ids=["zero_dir", "nan_origin", "inf_dir", "inf_origin", "nan_t_min", "nan_t_max", "min_above_max"])
def test_invalid_rays_are_flagged_and_miss(o, d, lo, hi):
    for flags in (0, abi.RAY_ANY_HIT, abi.RAY_CULL_BACK):
        assert _is_miss(_one(o, d, ONE, flags, lo, hi), abi.RAY_INVALID)


def test_a_nan_corner_is_a_miss_and_hides_nothing():
    h = _one((0.25, 0.25, 2), (0, 0, -1), [[[0, 0, 1], [np.nan, 0, 1], [0, 1, 1]], ONE[0]])
    assert h["flags"] == 1 and h["triangle"] == 1


def test_no_rays_or_no_triangles():
    assert len(engine.ray_triangles(np.zeros(0, dtype=abi.RAY), np.asarray(ONE, dtype=np.float32))) == 0
    hits = engine.ray_triangles(abi.make_rays([(0.25, 0.25, 2)], [(0, 0, -1)]), np.zeros((0, 3, 3), dtype=np.float32))
    assert _is_miss(hits[0])
    L = engine.lib()
    assert L.zr_ray_triangles(None, 0, None, 0, 0, None) == 0 and L.zr_ray_triangles(None, 1, None, 0, 0, None) == abi.ERR_ARG
    r = abi.make_rays([(0, 0, 1)], [(0, 0, -1)])
    h = np.zeros(1, dtype=abi.RAY_RECORD)
    assert L.zr_ray_triangles(r.ctypes.data, 1, None, 1, 0, h.ctypes.data) == abi.ERR_ARG           # triangles promised, none given
    assert L.zr_ray_triangles(r.ctypes.data, 1, None, 0, 8, h.ctypes.data) == abi.ERR_ARG           # an unknown flag bit


# ---- the stand-alone program

def test_rule_cases_under_the_sanitizers(check_exe):
    exe, _ = check_exe
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert re.fullmatch(r"cases \d+ failed 0", run.stdout.splitlines()[-1])


def test_two_compilers_give_the_same_bytes(check_exe):
    """the library's zr_ray_triangles (hipcc's host side) and the stand-alone program (g++) on the sphere cluster and on the grid's edges,
    every query flag: the same records, byte for byte"""
    exe, tmp = check_exe
    draws = rcc.draws_of(rcc.sphere_cluster())
    tris = rcc.world_f32(draws, np.eye(4))[::6].copy()
    rays = rcc.rays_at_triangles(np.random.default_rng(2), tris, 300)
    gtris, grays, _ = rcc.dyadic_grid_rays(100)
    for k, (t, r) in enumerate(((tris, rays), (gtris, grays))):
        for flags in (0, abi.RAY_CULL_BACK, abi.RAY_ANY_HIT):
            src, dst = tmp / ("in%d_%d.bin" % (k, flags)), tmp / ("out%d_%d.bin" % (k, flags))
            src.write_bytes(np.array([len(r), len(t), flags, 0], dtype=np.uint32).tobytes() + r.tobytes() + np.ascontiguousarray(t, dtype=np.float32).tobytes())
            subprocess.check_call([exe, str(src), str(dst)])
            assert dst.read_bytes() == engine.ray_triangles(r, t, flags).tobytes(), (k, flags)
