"""The deliveries whose kernel launches tests/test_gpu_wire_launches.py observes: run as a program of its own under a kernel trace.

First tests/delivery_launch_probe.py's whole run with a wire style SET on every context it makes but no wire stage asked for: every
existing call must launch what it always did (its EXPECTED).  Then one context more, per frame the staged calls of CALLS, with a
zr_finish behind each.  Prints delivery_launch_probe's line and then `staged <FRAMES> <calls per frame>`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import delivery_launch_probe as base

FRAMES = base.FRAMES
W, H = base.W, base.H
WIRE, HL, SCALE = ["k_wire_apply"], base.HL, base.SCALE
# (call, stages, scale) -> the kernels it launches, in order (stages: 1 wire, 2 highlight; the probe's contexts have no overlay list)
CALLS = [
    ("read_color_staged", 0, 1, []), ("read_color_staged", 1, 1, WIRE), ("read_color_staged", 1, 2, WIRE + SCALE),
    ("read_color_staged", 3, 1, WIRE + HL), ("read_color_staged", 7, 3, WIRE + HL + SCALE), ("read_color_staged", 2, 2, HL + SCALE),
    ("copy_frame_staged_async", 0, 1, SCALE), ("copy_frame_staged_async", 1, 1, WIRE), ("copy_frame_staged_async", 3, 2, WIRE + HL + SCALE),
]
EXPECTED = [k for _, _, _, ks in CALLS for k in ks]


def main():
    import torch
    from independent_scenes import _lights
    from zeldaengine_amd import abi, engine
    import highlight_cases as hc
    import test_gpu_highlight as hl

    made = hl._Host.__init__

    def with_a_wire_style(self, *a, **kw):
        made(self, *a, **kw)
        self.r.set_wire_style(rgba=(9, 9, 9, 255), width_256=700, flags=abi.WIRE_SELECTED)
    hl._Host.__init__ = with_a_wire_style
    base.main()
    a = hl._Host(engine, _lights(1, 4), W, H)
    a.select(hc.SETS["odd_box"])
    for f in range(FRAMES):
        a.move(0, 0.1)
        a.frame()
        a.r.finish()
        for call, stages, s, _ in CALLS:
            if call.startswith("copy_"):
                dest = hl._Dest(-(-W // s), -(-H // s))
                a.r.copy_frame_staged_async(stages, s, dest.ptr())
                a.r.finish()
                dest.read()
            else:
                a.r.read_color_staged(stages, s)
                a.r.finish()
    a.close()
    torch.cuda.synchronize()
    print("staged %d %d" % (FRAMES, len(CALLS)), flush=True)


if __name__ == "__main__":
    main()
