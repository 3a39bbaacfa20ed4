"""QOIX encode throughput (gamut_hip_qoix_encode_batch_device), one JSON line per batch, appended to profiles/qoix_encode_bench.jsonl.

    python tools/qoix_encode_bench.py [--images 1024] [--steps 5] [--warmup 2] [--json profiles/qoix_encode_bench.jsonl]

1920x1080 frames resident in HBM -> files in HBM, mode 0 (the reference's choice between the stored and the LZ4 file): rgb8 and rgba8,
photo-like and flat content from tests/qoix_gen.py.  With GAMUT_HIP_QOIX_TIMING=1 (set here) the call brackets its three launches with
events: the "kernel" figure and one per stage (ops, LZ4, the choice).  The whole call (upload of the image records, the length
read-back and the wait inside) is reported beside them, from the same calls: medians of `steps` calls after `warmup` calls.  Two
yardsticks from the same process: gamut_hip_qoi_encode_batch_device on the same pixels, and the C restatement of the reference
(tests/c/qoix_write_ref.c) on one host core -- the median of 5 warm encodes of one frame, also stated x 1/16 for the 16 cores a GPU
box grants.  Every batch is checked against that restatement on its first and last image before it is timed."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "qoix_encode_bench.jsonl"))
    a = ap.parse_args()
    os.environ["GAMUT_HIP_QOIX_TIMING"] = "1"                          # read once by the library, at its first encode call
    import torch
    import qoix_gen
    import qoix_write_ref_c
    from gamut_amd import _capi
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(**kw):
        rows.append(json.dumps(dict(tool="qoix_encode_bench", width=W, height=H, **kw)))
        print(rows[-1], flush=True)

    def calls(run, getters=()):
        """warmup + steps calls -> (median call ms, min call ms, [median of each getter])"""
        t, g = [], []
        for _ in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); run(); torch.cuda.synchronize(); t.append(1e3 * (time.perf_counter() - t0))
            g.append([f() for f in getters])
        t, g = t[a.warmup:], np.array(g[a.warmup:], np.float64).reshape(a.steps, len(getters))
        return float(np.median(t)), min(t), [float(x) for x in np.median(g, axis=0)]

    n = a.images
    for name, px in (("rgb8 photo-like", qoix_gen.photo_like(W, H, 3, 101)), ("rgba8 photo-like", qoix_gen.photo_like(W, H, 4, 102)),
                     ("rgb8 flat", qoix_gen.flat_image(W, H, 3, 103)), ("rgba8 flat", qoix_gen.flat_image(W, H, 4, 104))):
        px = np.ascontiguousarray(px)
        ch = px.shape[2]
        fb = W * H * ch
        want = qoix_write_ref_c.encode(px, 0)
        t = []
        for _ in range(6):                                              # the C restatement on one host core: 1 cold + 5 warm
            t0 = time.perf_counter(); qoix_write_ref_c.encode(px, 0); t.append(time.perf_counter() - t0)
        host_ms = 1e3 * float(np.median(t[1:]))
        s = torch.from_numpy(px.reshape(-1)).to(dev).repeat(n)
        ptrs = (C.c_void_p * n)(*[s.data_ptr() + i * fb for i in range(n)]); pitch = (C.c_int64 * n)(*([W * ch] * n))
        lens = (C.c_int64 * n)(); st = (C.c_int * n)()
        # ---- yardstick: the QOI encoder on the same pixels
        qd = (_capi.QoiDesc * n)(*[_capi.QoiDesc(W, H, ch, 0) for _ in range(n)])
        slot = (L.gamut_hip_qoi_encode_bound(C.byref(qd[0])) + 255) // 256 * 256
        out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
        offs = (C.c_int64 * n)(*[i * slot for i in range(n)])
        qoi_ms, qoi_min, _ = calls(lambda: _capi.check(L.gamut_hip_qoi_encode_batch_device(ptrs, pitch, qd, n, offs, out.data_ptr(), lens, st, stream)))
        qoi_bytes = int(lens[0])
        del out
        # ---- the QOIX encoder
        xd = (_capi.QoixDesc * n)(*[_capi.QoixDesc(W, H, ch, 0, 0, 1.0, 96.0) for _ in range(n)])
        slot = (L.gamut_hip_qoix_encode_bound(C.byref(xd[0])) + 255) // 256 * 256
        out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
        offs = (C.c_int64 * n)(*[i * slot for i in range(n)])
        run = lambda: _capi.check(L.gamut_hip_qoix_encode_batch_device(ptrs, pitch, xd, n, offs, out.data_ptr(), lens, st, stream))
        run()
        assert list(lens) == [len(want)] * n, "encode length"
        for i in (0, n - 1):
            assert out[i * slot:i * slot + len(want)].cpu().numpy().tobytes() == want, "encode parity"
        ms, mn, (km, s0, s1, s2) = calls(run, [L.gamut_hip_qoix_last_encode_kernel_ms] + [lambda k=k: L.gamut_hip_qoix_last_encode_stage_ms(k) for k in range(3)])
        emit(batch="encode " + name, images=n, kernel_ms=round(km, 3), call_ms=round(ms, 3), call_ms_min=round(mn, 3),
             stage_ms=dict(ops=round(s0, 3), lz4=round(s1, 3), choice=round(s2, 3)), file_bytes=len(want), lz4_file=int(want[16]),
             mpx_per_s=round(n * W * H / ms / 1e3, 1), qoi_encode_call_ms_same_pixels=round(qoi_ms, 3), qoi_encode_call_ms_min=round(qoi_min, 3),
             qoi_file_bytes=qoi_bytes, host_one_core_ms_per_frame=round(host_ms, 3), host_one_core_ms_per_batch=round(host_ms * n, 1),
             host_16_cores_ms_per_batch=round(host_ms * n / 16, 1))
        del out, s
    if a.json:
        with open(a.json, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
