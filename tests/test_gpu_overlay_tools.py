"""The overlay seen from outside the library: which kernels every form of delivery launches once a context has an overlay list
(tests/overlay_launch_probe.py, run once as a child process under `rocprofv3 --kernel-trace` with a time limit of its own, as
tests/test_gpu_delivery_launches.py runs its probe), and the native driver's --overlay."""
import csv
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import overlay_launch_probe as probe
from zeldaengine_amd import build as zbuild

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = ("k_frame_scale", "k_highlight_", "k_delta_", "k_overlay_")


def test_the_launches_with_an_overlay_list_set(gpu_engine, tmp_path):
    """the new calls launch k_overlay_setup then k_overlay_apply, with the highlight's two launches ahead of them where highlight = 1 and
    k_frame_scale behind at a scale above 1; every call of DESIGN.md section 5's table launches exactly what the table says although the
    context has a list; the deliveries of changes launch the two only with overlay delivery on"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    assert os.path.exists(rocprof), "rocprofv3 is what observes the launches"
    out = tmp_path / "trace"
    env = dict(os.environ, TMPDIR=str(tmp_path))
    run = subprocess.run(["timeout", "-k", "10", "150", rocprof, "--kernel-trace", "--output-format", "csv", "-d", str(out), "-o", "probe", "--",
                          sys.executable, os.path.join(ROOT, "tests", "overlay_launch_probe.py")],
                         cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=180)
    text = run.stdout.decode(errors="replace")
    assert run.returncode == 0, text[-4000:]
    assert "delivered %d %d" % (probe.FRAMES, probe.N_CALLS) in text, text[-4000:]
    traces = glob.glob(str(out / "**" / "*kernel_trace.csv"), recursive=True)
    assert len(traces) == 1, traces
    rows = [r for r in csv.DictReader(open(traces[0])) if any(k in r["Kernel_Name"] for k in OBSERVED)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"].replace("void ", "").split("<")[0].split("(")[0] for r in rows]
    assert names == probe.EXPECTED * probe.FRAMES, names


def _box_rows(g, obj, instance):
    """the twelve edges of an instance's bounds as tools/zelda_headless --overlay-box computes them: the box of the mesh's vertices through
    the vertex stage's instance transform, in double precision, in the tool's order of operations"""
    import math
    mesh, inst = g.object_get_instances(obj)
    v = g.mesh_get_vertices(mesh)["Position"].astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    R, t, sc = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0], 1.0
    if inst is not None and instance < len(inst):
        I = inst[instance]
        rot = [float(a) for a in I["InstanceRotation"]]
        cx, sx, cy, sy, cz, sz = math.cos(rot[0]), math.sin(rot[0]), math.cos(rot[1]), math.sin(rot[1]), math.cos(rot[2]), math.sin(rot[2])
        mx, my, mz = [cx, 0, sx, 0, 1, 0, -sx, 0, cx], [cy, sy, 0, -sy, cy, 0, 0, 0, 1], [1, 0, 0, 0, cz, sz, 0, -sz, cz]

        def mul(A, B):
            return [A[r] * B[c * 3] + A[3 + r] * B[c * 3 + 1] + A[6 + r] * B[c * 3 + 2] for c in range(3) for r in range(3)]
        R, sc, t = mul(mul(mz, my), mx), float(I["InstancePScale"]), [float(a) for a in I["InstancePosition"]]
    corner = []
    for i in range(8):
        p = [float((hi if i & (1 << k) else lo)[k]) * sc for k in range(3)]
        corner.append([float(np.float32(p[0] * R[j * 3] + p[1] * R[j * 3 + 1] + p[2] * R[j * 3 + 2] + t[j])) for j in range(3)])
    return [tuple(corner[i]) + tuple(corner[i | b]) + (255, 220, 0, 255, 0) for i in range(8) for b in (1, 2, 4) if not i & b]


def test_headless_overlay_box_draws_the_picked_instances_bounds(gpu_engine, tmp_path):
    """tools/zelda_headless --pick ... --overlay-box: a box per printed hit, and the written image is Renderer.read_color_overlaid's for
    the boxes' edges under the tool's style"""
    import json
    from test_gpu_native_host import H, SD, W, _content_tree
    root = str(tmp_path)
    _content_tree(root)
    exe = zbuild.build_headless()
    rect = (W // 4, H // 4, W // 2, H // 2)
    ppm = os.path.join(root, "box.ppm")
    out = subprocess.run([exe, "--root", root, "--world", "Content/World.json", "--size", "%dx%d" % (W, H), "--shadow", str(SD), "--frames", "2",
                          "--pick", "%d,%d,%d,%d" % rect, "--overlay-box", "--out", ppm], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode(errors="replace")
    assert out.returncode == 0, text
    hits = [json.loads(l) for l in text.splitlines() if l.startswith("{")]
    boxes = [tuple(int(x) for x in l.split()[1:]) for l in text.splitlines() if l.startswith("overlay-box ")]
    assert hits and boxes == [(h["object"], h["instance"]) for h in hits]
    g = gpu_engine.Renderer(W, H, SD)
    try:
        g.set_asset_root(root)
        g.world_load_file("Content/World.json")
        g.overlay_style(depth_bias=0.0, hidden_opacity=85)
        rows = []
        for o, i in boxes:
            rows += _box_rows(g, o, i)
        assert len(rows) == 12 * len(boxes)
        g.overlay_set(rows)
        for f in range(2):
            g.world_update_uniforms(0.0, 0.0, 0.016 * f)
            g.render()
        want = g.read_color_overlaid(1)
        header = ("P6\n%d %d\n255\n" % (W, H)).encode()
        assert open(ppm, "rb").read() == header + want[..., :3].tobytes()
        assert int((want != g.color()).any(axis=2).sum()) >= 12
    finally:
        g.close()


def test_headless_overlay_writes_the_overlaid_image(gpu_engine, tmp_path):
    """tools/zelda_headless --overlay FILE: the written image is the one Renderer.read_color_overlaid returns for the file's list,
    plain and through --delta-packed --scale 2"""
    from test_gpu_native_host import H, SD, W, _content_tree
    root = str(tmp_path)
    _content_tree(root)
    exe = zbuild.build_headless()
    rows = [(-3.0, -3.0, 0.0, 3.0, 3.0, 2.0, 255, 0, 0, 255, 1), (-3.0, 3.0, 0.5, 3.0, -3.0, 0.5, 0, 255, 0, 160, 0), (0.0, 0.0, -2.0, 0.0, 0.0, 4.0, 0, 0, 255, 255, 0),
            (-50.0, 0.25, 0.25, 50.0, 0.25, 0.25, 255, 255, 0, 128, 0), (2.0, -2.0, 0.0, 2.0, 2.0, 3.0, 255, 255, 255, 200, 1)]
    path = os.path.join(root, "lines.txt")
    with open(path, "w") as f:
        f.write("# ax ay az bx by bz r g b a flags\n\n" + "".join(" ".join(repr(v) for v in r) + "\n" for r in rows))
    images = {}
    for mode, extra in (("plain", []), ("packed2", ["--delta-packed", "--scale", "2"])):
        ppm = os.path.join(root, mode + ".ppm")
        out = subprocess.run([exe, "--root", root, "--world", "Content/World.json", "--size", "%dx%d" % (W, H), "--shadow", str(SD), "--frames", "2",
                              "--overlay", path, "--out", ppm] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert out.returncode == 0, out.stdout.decode(errors="replace")
        images[mode] = open(ppm, "rb").read()
    g = gpu_engine.Renderer(W, H, SD)
    try:
        g.set_asset_root(root)
        g.world_load_file("Content/World.json")
        g.overlay_set(rows)
        for f in range(2):
            g.world_update_uniforms(0.0, 0.0, 0.016 * f)
            g.render()
        for mode, s in (("plain", 1), ("packed2", 2)):
            want = g.read_color_overlaid(s)
            header = ("P6\n%d %d\n255\n" % (want.shape[1], want.shape[0])).encode()
            assert images[mode] == header + want[..., :3].tobytes(), mode
        assert not np.array_equal(g.read_color_overlaid(1), g.color())
    finally:
        g.close()
