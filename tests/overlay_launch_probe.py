"""The deliveries whose kernel launches tests/test_gpu_overlay_tools.py observes: run as a program of its own under a kernel trace.

tests/delivery_launch_probe.py's contexts and calls (its CALLS and DELTAS, unchanged), every context WITH AN OVERLAY LIST SET - so each
existing call must still launch exactly what DESIGN.md's table says, and nothing of the overlay - followed per frame by the new calls
(OVERLAID) and by two more deliveries of changes that carry the lines (OV_DELTAS).  EXPECTED is what one such frame must launch, call by
call.  Prints one line, `delivered <FRAMES> <calls per frame>`, when all of them went through."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import delivery_launch_probe as base      # noqa: E402

FRAMES, W, H = base.FRAMES, base.W, base.H
OV = ["k_overlay_setup", "k_overlay_apply"]
# (scale, highlight) -> the kernels of zr_read_color_overlaid and of zr_copy_frame_overlaid_async alike
OVERLAID = [(1, False, OV), (2, False, OV + base.SCALE), (1, True, base.HL + OV), (3, True, base.HL + OV + base.SCALE)]
# (delta scale, packed, highlighted) with overlay delivery on; made twice per frame, host form then device form
OV_DELTAS = [(1, False, False, OV + base.RAW), (2, True, True, base.HL + OV + base.SCALE + base.PACKED)]
EXPECTED = (base.EXPECTED[:sum(len(ks) for _, _, ks in base.CALLS)] + [k for _, _, ks in OVERLAID for k in ks * 2] +
            [k for _, _, _, ks in base.DELTAS for k in ks * 2] + [k for _, _, _, ks in OV_DELTAS for k in ks * 2])
N_CALLS = len(base.CALLS) + 2 * len(OVERLAID) + 2 * len(base.DELTAS) + 2 * len(OV_DELTAS)


def main():
    import torch
    from independent_scenes import _lights
    from zeldaengine_amd import abi, engine
    import highlight_cases as hc
    import overlay_cases as oc
    import test_gpu_highlight as hl
    import test_gpu_overlay as ov

    lights = _lights(1, 4)

    def host(delta=None, overlay=False):
        h = hl._Host(engine, lights, W, H)
        h.select(hc.SETS["odd_box"])
        h.frame()
        h.r.overlay_set(oc.lists(ov._pvm(h.r), W, H)["slopes"])
        if delta:
            scale, packed, highlighted = delta
            h.r.set_frame_delta_overlay(overlay)
            h.delta_on(scale, abi.FRAME_DELTA_PACKED if packed else 1, highlight=highlighted)
        return h

    a = host()
    deltas = [(host(d[:3], False), 2 if d[1] else 0) for d in base.DELTAS] + [(host(d[:3], True), 2 if d[1] else 0) for d in OV_DELTAS]
    for h in [a] + [d for d, _ in deltas]:
        h.r.finish()
    print("frames begin", flush=True)
    for f in range(FRAMES):
        a.move(0, 0.1)
        a.frame()
        a.r.finish()
        for call, s, _ in base.CALLS:
            if call.startswith("copy_"):
                dest = hl._Dest(-(-W // s), -(-H // s))
                getattr(a.r, call)(s, dest.ptr())
                a.r.finish()
                dest.read()
            else:
                getattr(a.r, call)(s)
                a.r.finish()
        for s, highlighted, _ in OVERLAID:
            a.r.read_color_overlaid(s, highlighted)
            a.r.finish()
            dest = hl._Dest(-(-W // s), -(-H // s))
            a.r.copy_frame_overlaid_async(s, highlighted, dest.ptr())
            a.r.finish()
            dest.read()
        for d, form in deltas:
            d.move(0, 0.1)                   # (so that a delivery lists something)
            d.frame()
            d.r.finish()
            _, hd = d.deliver_form(form)         # the host form
            d.r.finish()
            assert hd["n_tiles"] > 0 and hd["serial"] == 2 * f + 1, hd
            _, hd = d.deliver_form(form + 1)     # the device form
            assert hd["serial"] == 2 * f + 2, hd
    for d, _ in deltas:
        d.close()
    a.close()
    torch.cuda.synchronize()
    print("delivered %d %d" % (FRAMES, N_CALLS), flush=True)


if __name__ == "__main__":
    main()
