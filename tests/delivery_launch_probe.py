"""The deliveries whose kernel launches tests/test_gpu_delivery_launches.py observes: run as a program of its own under a kernel trace.

One context at W x H with tests/highlight_cases.py's scene, id capture on and a non-empty set, and four more that deliver changes (raw;
raw at scale 2; raw highlighted; packed, highlighted, at scale 2).  Per rendered frame every form of delivery is called once, in the order
of CALLS, with a zr_finish behind each; every delivery of changes in its host form and then in its device form.  EXPECTED is what one such
frame must launch, call by call.  Prints one line, `delivered <FRAMES> <calls per frame>`, when all of them went through."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FRAMES = 2
W, H = 66, 34

HL = ["k_highlight_mask", "k_highlight_apply"]
SCALE = ["k_frame_scale"]
RAW = ["k_delta_mark", "k_delta_pack"]
PACKED = ["k_delta_mark", "k_delta_measure", "k_delta_encode"]

# (call, scale) -> the kernels it launches, in order
CALLS = [
    ("color_scaled", 1, []), ("color_scaled", 2, SCALE), ("color_scaled", 3, SCALE),
    ("copy_frame_scaled_async", 1, SCALE), ("copy_frame_scaled_async", 2, SCALE),
    ("color_highlighted", 1, HL), ("color_highlighted", 2, HL + SCALE),
    ("copy_frame_highlighted_async", 1, HL), ("copy_frame_highlighted_async", 2, HL + SCALE),
]
# (delta scale, packed, highlighted) -> one delivery's kernels; made twice per frame, host form then device form
DELTAS = [
    (1, False, False, RAW), (2, False, False, SCALE + RAW), (1, False, True, HL + RAW), (2, True, True, HL + SCALE + PACKED),
]
EXPECTED = [k for _, _, ks in CALLS for k in ks] + [k for _, _, _, ks in DELTAS for k in ks * 2]
N_CALLS = len(CALLS) + 2 * len(DELTAS)


def main():
    import torch
    from independent_scenes import _lights
    from zeldaengine_amd import abi, engine
    import highlight_cases as hc
    import test_gpu_highlight as hl

    lights = _lights(1, 4)
    a = hl._Host(engine, lights, W, H)
    a.select(hc.SETS["odd_box"])
    deltas = []
    for scale, packed, highlighted, _ in DELTAS:
        d = hl._Host(engine, lights, W, H)
        d.select(hc.SETS["odd_box"])
        d.delta_on(scale, abi.FRAME_DELTA_PACKED if packed else 1, highlight=highlighted)
        deltas.append((d, 2 if packed else 0))
    for f in range(FRAMES):
        a.move(0, 0.1)
        a.frame()
        a.r.finish()
        for call, s, _ in CALLS:
            if call.startswith("copy_"):
                dest = hl._Dest(-(-W // s), -(-H // s))
                getattr(a.r, call)(s, dest.ptr())
                a.r.finish()
                dest.read()
            else:
                getattr(a.r, call)(s)
                a.r.finish()
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
