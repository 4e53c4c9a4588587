"""Which kernels every form of delivery launches, observed from outside the library: tests/delivery_launch_probe.py runs once as a child
process under `rocprofv3 --kernel-trace` (a time limit of its own), and the trace's k_frame_scale, k_highlight_* and k_delta_* dispatches
are read back in the order they started.

A delivery is the frame, highlighted or not (k_highlight_mask, k_highlight_apply), filtered or not (k_frame_scale), and then a form: the
whole frame (no further launch), changed tiles raw (k_delta_mark, k_delta_pack) or packed (k_delta_mark, k_delta_measure,
k_delta_encode).  DESIGN.md section 5 has the table call by call; the probe's EXPECTED restates it."""
import csv
import glob
import os
import shutil
import subprocess
import sys

import pytest

import delivery_launch_probe as probe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBSERVED = ("k_frame_scale", "k_highlight_", "k_delta_")


def test_every_form_of_delivery_makes_the_launches_of_the_table(gpu_engine, tmp_path):
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    assert os.path.exists(rocprof), "rocprofv3 is what observes the launches"
    out = tmp_path / "trace"
    env = dict(os.environ, TMPDIR=str(tmp_path))
    run = subprocess.run(["timeout", "-k", "10", "120", rocprof, "--kernel-trace", "--output-format", "csv", "-d", str(out), "-o", "probe", "--",
                          sys.executable, os.path.join(ROOT, "tests", "delivery_launch_probe.py")],
                         cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=150)
    text = run.stdout.decode(errors="replace")
    assert run.returncode == 0, text[-4000:]
    assert "delivered %d %d" % (probe.FRAMES, probe.N_CALLS) in text, text[-4000:]
    traces = glob.glob(str(out / "**" / "*kernel_trace.csv"), recursive=True)
    assert len(traces) == 1, traces
    rows = [r for r in csv.DictReader(open(traces[0])) if any(k in r["Kernel_Name"] for k in OBSERVED)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"].replace("void ", "").split("<")[0].split("(")[0] for r in rows]
    assert names == probe.EXPECTED * probe.FRAMES, names
