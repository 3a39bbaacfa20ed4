"""QOI-Plane encode throughput (gamut_hip_qoix_encode_batch_device with 1 / 2 channels, gamut_hip_qoix_set_plane(1)), one JSON line
per batch, appended to profiles/qoix_plane_encode_bench.jsonl.

    python tools/qoix_plane_encode_bench.py [--images 1024] [--steps 5] [--warmup 2] [--json profiles/qoix_plane_encode_bench.jsonl]

1920x1080 frames resident in HBM -> files in HBM: photo-like l8, photo-like la8 and flat l8 from tests/qoiplane_gen.py, in mode 0 (the
reference's choice between the stored and the LZ4 file) and mode 1 (stored only).  With GAMUT_HIP_QOIX_TIMING=1 (set here) the call
brackets its launches with events: the grey encoder's three stages (count, scan, write), then LZ4 and the choice.  The whole call
(upload of the image records, the length read-back and the wait inside) is reported beside them, from the same calls: medians of
`steps` calls after `warmup` calls.  Yardsticks from the same process: k_qxenc_ops (the colour encoder, a wave per image) on an rgb8
version of the photo-like picture, k_convert_vec rgb8 -> rgba8 on the same frame count, and the C restatement of the reference
(tests/c/qoiplane_write_ref.c, LZ4 from tests/c/qoix_write_ref.c) on one host core -- the median of 5 warm encodes of one frame.  Every
batch is checked against that restatement on its first and last image before it is timed."""
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
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "qoix_plane_encode_bench.jsonl"))
    a = ap.parse_args()
    os.environ["GAMUT_HIP_QOIX_TIMING"] = "1"                          # read once by the library, at its first encode call
    import torch
    import oracle_lib as O
    import qoiplane_gen as P
    import qoiplane_write_ref_c as ref
    import qoix_write_ref_c
    from gamut_amd import _capi
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    L.gamut_hip_qoix_set_plane(1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(**kw):
        rows.append(json.dumps(dict(tool="qoix_plane_encode_bench", width=W, height=H, segment=L.gamut_hip_qoix_plane_encode_segment(), **kw)))
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

    def host_ms(f):
        t = []
        for _ in range(6):                                              # one host core: 1 cold + 5 warm
            t0 = time.perf_counter(); f(); t.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(t[1:]))

    n = a.images
    photo = P.photo_like(W, H, 1, 101)
    # ---- yardstick: k_convert_vec rgb8 -> rgba8 on n frames
    rgb = np.ascontiguousarray(np.repeat(photo, 3, axis=2))
    rgb[..., 1] = np.roll(rgb[..., 1], 3, axis=1); rgb[..., 2] = np.roll(rgb[..., 2], 5, axis=0)        # three channels that differ
    src = torch.from_numpy(rgb.reshape(-1)).to(dev).repeat(n)
    dst = torch.empty(n * W * H * 4, dtype=torch.uint8, device=dev)
    ms, mn, _ = calls(lambda: _capi.check(L.gamut_hip_scanlines_convert_device(O.PT["rgb8"], src.data_ptr(), W * 3, W * H * 3, O.PT["rgba8"], dst.data_ptr(), W * 4,
                                                                                W * H * 4, W, H, n, stream)))
    emit(batch="yardstick k_convert_vec rgb8->rgba8", images=n, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(n * W * H / ms / 1e3, 1))
    del dst
    # ---- yardstick: k_qxenc_ops, the colour encoder's op kernel, on the same rgb8 frames (mode 1: ops alone)
    ptrs = (C.c_void_p * n)(*[src.data_ptr() + i * W * H * 3 for i in range(n)]); pitch = (C.c_int64 * n)(*([W * 3] * n))
    lens = (C.c_int64 * n)(); st = (C.c_int * n)()
    xd = (_capi.QoixDesc * n)(*[_capi.QoixDesc(W, H, 3, 0, 1, 1.0, 96.0) for _ in range(n)])
    slot = (L.gamut_hip_qoix_encode_bound(C.byref(xd[0])) + 255) // 256 * 256
    out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    offs = (C.c_int64 * n)(*[i * slot for i in range(n)])
    run = lambda: _capi.check(L.gamut_hip_qoix_encode_batch_device(ptrs, pitch, xd, n, offs, out.data_ptr(), lens, st, stream))
    run()
    want = qoix_write_ref_c.encode(rgb, 1)
    assert list(lens) == [len(want)] * n and out[:len(want)].cpu().numpy().tobytes() == want, "colour encode parity"
    ms, mn, (ops,) = calls(run, [lambda: L.gamut_hip_qoix_last_encode_stage_ms(0)])
    emit(batch="yardstick k_qxenc_ops rgb8 photo-like, stored", images=n, ops_ms=round(ops, 3), call_ms=round(ms, 3), call_ms_min=round(mn, 3), file_bytes=len(want),
         mpx_per_s=round(n * W * H / ms / 1e3, 1))
    del out, src
    # ---- the grey encoder
    for name, px in (("l8 photo-like", photo), ("la8 photo-like", P.photo_like(W, H, 2, 102)), ("l8 flat", P.flat_image(W, H, 1, 103))):
        px = np.ascontiguousarray(px)
        ch = px.shape[2]
        fb = W * H * ch
        s = torch.from_numpy(px.reshape(-1)).to(dev).repeat(n)
        ptrs = (C.c_void_p * n)(*[s.data_ptr() + i * fb for i in range(n)]); pitch = (C.c_int64 * n)(*([W * ch] * n))
        ref_stored_ms = host_ms(lambda: ref.stored(px))
        ref_file_ms = host_ms(lambda: ref.encode(px, 0))
        for mode in (1, 0):
            want = ref.encode(px, mode)
            xd = (_capi.QoixDesc * n)(*[_capi.QoixDesc(W, H, ch, 0, mode, 1.0, 96.0) for _ in range(n)])
            slot = (L.gamut_hip_qoix_encode_bound(C.byref(xd[0])) + 255) // 256 * 256
            out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
            offs = (C.c_int64 * n)(*[i * slot for i in range(n)])
            run = lambda: _capi.check(L.gamut_hip_qoix_encode_batch_device(ptrs, pitch, xd, n, offs, out.data_ptr(), lens, st, stream))
            run()
            assert list(lens) == [len(want)] * n, "encode length"
            for i in (0, n - 1):
                assert out[i * slot:i * slot + len(want)].cpu().numpy().tobytes() == want, "encode parity"
            getters = [lambda k=k: L.gamut_hip_qoix_last_plane_encode_stage_ms(k) for k in range(3)] + [lambda k=k: L.gamut_hip_qoix_last_encode_stage_ms(k) for k in (1, 2)]
            ms, mn, (t_count, t_scan, t_write, t_lz4, t_pick) = calls(run, getters)
            host = ref_file_ms if mode == 0 else ref_stored_ms
            emit(batch=f"encode {name}, mode {mode}", images=n, mode=mode, call_ms=round(ms, 3), call_ms_min=round(mn, 3),
                 stage_ms=dict(count=round(t_count, 3), scan=round(t_scan, 3), write=round(t_write, 3), lz4=round(t_lz4, 3), choice=round(t_pick, 3)),
                 count_plus_write_ms=round(t_count + t_write, 3), file_bytes=len(want), lz4_file=int(want[16]), output_bytes=n * len(want),
                 mpx_per_s=round(n * W * H / ms / 1e3, 1), host_one_core_ms_per_frame=round(host, 3), host_one_core_ms_per_batch=round(host * n, 1),
                 host_16_cores_ms_per_batch=round(host * n / 16, 1))
            del out
        del s
    if a.json:
        with open(a.json, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
