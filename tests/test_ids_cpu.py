"""Object identity of the last frame, the parts that need no GPU: the zr_hit layout in C, C++ and numpy, and the test-side reference
mapping (tests/ids_reference.py) held to the CPU oracle's shaded output, so that the GPU tests' reference is not a restatement of the
library's own numbering."""
import os
import subprocess

import numpy as np
import pytest

import ids_reference as idr
from independent_scenes import Scene, _lights
from zeldaengine_amd import abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["object", "instance", "pixels", "triangle", "x", "y", "depth", "reserved"]


@pytest.mark.parametrize("compiler,ext", [("gcc", "c"), ("g++", "cpp")])
def test_zr_hit_layout_in_c_and_cpp_matches_abi_hit(tmp_path, compiler, ext):
    src = tmp_path / ("hit." + ext)
    offs = "".join('printf(" %%zu", (size_t)offsetof(zr_hit, %s));' % f for f in FIELDS)
    src.write_text('#include "zelda_render.h"\n#include <stddef.h>\n#include <stdio.h>\n'
                   'int main(void){printf("%%zu", sizeof(zr_hit));%s return 0;}\n' % offs)
    exe = tmp_path / ("hit_" + ext)
    subprocess.check_call([compiler, "-std=c11" if ext == "c" else "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == 32 == abi.Hit.itemsize
    assert got[1:] == [abi.Hit.fields[f][1] for f in FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28]
    import ctypes as C
    assert [getattr(abi.HitC, f).offset for f in FIELDS] == got[1:] and C.sizeof(abi.HitC) == 32


def test_abi_version_is_seven():
    assert abi.ABI_VERSION == 7
    hdr = open(os.path.join(ROOT, "include", "zelda_render.h")).read()
    assert "#define ZR_ABI_VERSION 7u" in hdr and "int  zr_pick(" in hdr


def _tagged_scene():
    """objects whose SceneColor words differ: the emissive slot (5) carries the object's add-order index.  Instanced draws are added
    before and between non-instanced ones, so add order and draw order differ."""
    s = Scene()

    def tex(i):
        t = [(127, 127, 127, 255), (0, 0, 0, 255), (255, 255, 255, 255), (127, 127, 255, 255), (255, 255, 255, 255),
             (10 + 20 * i, 200 - 15 * i, 7 * i, 255), (255, 255, 255, 255)]
        return t
    s.add(scenes.uv_sphere(10, 5, 0.5), tex(0), scenes.generate_instances(30, 0.8, 4.0, 0.4, 1.0, seed=5))
    s.add(scenes.grid_plane(14.0, 3, 0.0), tex(1))
    s.add(scenes.box((0.5, 0.4, 0.6), (0.0, 0.0, 0.6)), tex(2), scenes.generate_instances(12, 1.0, 4.5, 0.5, 1.1, seed=6))
    s.add(scenes.box((0.8, 0.6, 0.5), (1.0, -1.2, 0.5)), tex(3))
    s.add(scenes.uv_sphere(12, 6, 0.7), tex(4), scenes.generate_instances(1, 0.0, 0.5, 1.0, 1.0, seed=9))
    return s, [tuple(tex(i)[5][:3]) for i in range(5)]


def _render_oracle(oracle_lib, s, W, H, cam):
    o = oracle_lib.Oracle(W, H, 256)
    s.load(o)
    d, p, sp = _lights(1, 2)
    o.update_uniforms(cam, d, p, sp, 0.0, 0.0, 0.0)
    o.render()
    return o


@pytest.mark.parametrize("W,H", [(192, 128), (257, 131)])
def test_reference_mapping_names_the_object_the_oracle_shaded(oracle_lib, W, H):
    s, emissive = _tagged_scene()
    o = _render_oracle(oracle_lib, s, W, H, abi.make_camera((5.0, 4.0, 3.0), (0.0, 0.0, 0.4), fov=60.0))
    vis = o.visibility().copy()
    sc = o.gbuffer(1).copy().view(np.uint32) & np.uint32(0xFFFFFF)
    items = idr.items_of_scene(s)
    m = idr.mapping(vis, items)
    cov = vis != idr.NO_ID
    assert cov.mean() > 0.3
    want = np.array([r | g << 8 | b << 16 for r, g, b in emissive], dtype=np.uint32)
    assert np.array_equal(sc[cov], want[m["object"][cov]])
    seen = set(np.unique(m["object"][cov]).tolist())
    assert seen == {0, 1, 2, 3, 4}, seen                   # every object won pixels: each one's numbering is checked
    # instances and triangles stay inside their object
    counts = [1 if inst is None else len(inst) for _, inst in items]
    assert (m["instance"][cov] < np.array(counts)[m["object"][cov]]).all()
    assert (m["triangle"][cov] < np.array([nt for nt, _ in items])[m["object"][cov]]).all()
    # slot coverage sums to the oracle's covered pixels, and the object plane is what the mapping says
    c = idr.coverage(vis, items)
    assert c.sum() == o.covered_pixels() == cov.sum()
    assert len(c) == sum(counts)
    plane = idr.object_plane(vis, items)
    assert (plane[~cov] == idr.NO_ID).all()


def test_reference_mapping_negative_control(oracle_lib):
    """numbering the draws in add order (ignoring that non-instanced draws go first) must disagree with the oracle's shading"""
    s, emissive = _tagged_scene()
    o = _render_oracle(oracle_lib, s, 192, 128, abi.make_camera((5.0, 4.0, 3.0), (0.0, 0.0, 0.4), fov=60.0))
    vis = o.visibility().copy()
    sc = o.gbuffer(1).copy().view(np.uint32) & np.uint32(0xFFFFFF)
    items = idr.items_of_scene(s)
    bases = np.cumsum([0] + [nt * (1 if inst is None else len(inst)) for nt, inst in items])[:-1]
    cov = vis != idr.NO_ID
    wrong = np.clip(np.searchsorted(bases, vis.astype(np.int64), side="right") - 1, 0, len(items) - 1)
    want = np.array([r | g << 8 | b << 16 for r, g, b in emissive], dtype=np.uint32)
    assert not np.array_equal(sc[cov], want[wrong[cov]])


def test_reference_pick_on_a_synthetic_plane():
    items = [(2, None), (3, [0, 0])]          # object 0: 2 triangles, non-instanced; object 1: 3 triangles, two instances
    # draw order: object 0 (prims 0-1), then object 1 (prims 2-7: instance 0 = 2-4, instance 1 = 5-7)
    vis = np.full((4, 6), idr.NO_ID, dtype=np.uint32)
    vis[0, :3] = 1; vis[1, 1:4] = 6; vis[2, 2] = 3; vis[3, 5] = 7
    depth = np.ones((4, 6), np.float32)
    depth[0, :3] = [0.5, 0.4, 0.4]; depth[1, 1:4] = [0.3, 0.2, 0.6]; depth[2, 2] = 0.7; depth[3, 5] = 0.1
    hits, total = idr.pick(vis, depth, items, 0, 0, 100, 100)
    assert total == 3
    assert hits[0] == (1, 1, 4, 2, 5, 3, np.float32(0.1)) or hits[0][:6] == (1, 1, 4, 2, 5, 3)
    assert [h[:2] for h in hits] == [(1, 1), (0, 0), (1, 0)]
    assert hits[1][2:6] == (3, 1, 1, 0)        # 3 pixels, triangle 1, nearest (1, 0): ties to the least y*W + x
    assert idr.pick(vis, depth, items, 6, 0, 1, 1) == ([], 0)
    assert idr.coverage(vis, items).tolist() == [3, 1, 4]
