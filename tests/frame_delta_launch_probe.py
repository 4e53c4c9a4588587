"""The deliveries whose kernel launches tests/test_gpu_frame_delta_launches.py observes: run as a program of its own under a kernel trace.

A context in mode 1 (zr_set_frame_delta(ctx, 1)) makes RAW raw deliveries, host and device form in turn; a context in mode 3
(ZR_FRAME_DELTA_PACKED) makes PACKED packed deliveries, then RAW_BESIDE raw ones.  Prints one line, `delivered <RAW> <PACKED> <RAW_BESIDE>`,
when all of them went through."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RAW, PACKED, RAW_BESIDE = 5, 3, 2
W, H = 257, 131


def main():
    import torch
    from independent_scenes import _lights
    from zeldaengine_amd import abi, engine
    import test_gpu_frame_delta as raw
    import test_gpu_frame_delta_packed as packed

    lights = _lights(1, 4)

    def deliver(h, k, form):
        h.move(0, 0.1)                       # (so that a delivery lists something)
        h.frame()
        if k % 2 == 0:
            (h.r.read_frame_delta if form == "raw" else h.r.read_frame_delta_packed)()
        else:
            s = (raw._DeviceSet if form == "raw" else packed._DeviceSet)(h.total)
            s.enqueue(h.r)
            h.r.finish()
            assert s.read()[-1]["n_tiles"] > 0

    a = raw._Host(engine, lights, W, H, delta=False)
    a.r.set_frame_delta(1)
    for k in range(RAW):
        deliver(a, k, "raw")
    a.close()
    b = raw._Host(engine, lights, W, H, delta=False)
    b.r.set_frame_delta(abi.FRAME_DELTA_PACKED)
    for k in range(PACKED):
        deliver(b, k, "packed")
    for k in range(RAW_BESIDE):
        deliver(b, k, "raw")
    b.close()
    torch.cuda.synchronize()
    print("delivered %d %d %d" % (RAW, PACKED, RAW_BESIDE), flush=True)


if __name__ == "__main__":
    main()
