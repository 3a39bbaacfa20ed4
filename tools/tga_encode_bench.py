"""TGA encode throughput (gamut_hip_tga_encode_batch_device), one JSON line per batch, appended to profiles/tga_encode_bench.jsonl.

    python tools/tga_encode_bench.py [--images 1024] [--steps 3] [--warmup 1] [--json profiles/tga_encode_bench.jsonl]

1920x1080 frames resident in HBM -> files in HBM: rgb8 photo-like, rgba8 photo-like, rgba8 flat (tiles of one colour), rgb8 without
run-length packets.  With GAMUT_HIP_TGA_TIMING=1 (set here) the call brackets its three launches with events: the "kernel" figures,
and one per stage (row lengths, offsets, write).  The whole call (upload of the image records, the length read-back and the wait
inside) is reported beside them.  The fraction of 8 TB/s is counted on algorithmic bytes: pixel bytes read plus file bytes written,
each ONCE (the encoder reads the pixels twice; that shows as a lower fraction, as it should).  The yardstick is k_convert_vec
rgb8 -> rgba8 (gamut_hip_scanlines_convert_device) on the same frame count in the same process; the host figure is the C
restatement of the reference (tests/c/tga_write_ref.c) on one core, the median of 5 warm encodes of one frame.  Every batch is
checked against that restatement on its first and last image before it is timed."""
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


def timed(run, steps, warmup, sync):
    for _ in range(warmup):
        run()
    sync()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter(); run(); sync(); t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "tga_encode_bench.jsonl"))
    a = ap.parse_args()
    os.environ["GAMUT_HIP_TGA_TIMING"] = "1"                           # read once by the library, at its first encode call
    import torch
    import oracle_lib as O
    import tga_write_ref_c
    from gamut_amd import _capi, synth
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(**kw):
        rows.append(json.dumps(dict(tool="tga_encode_bench", width=W, height=H, **kw)))
        print(rows[-1], flush=True)

    n = a.images
    photo = np.ascontiguousarray(synth.photo_rgb(W, H, 101))
    photo_a = np.dstack([photo, np.full((H, W), 255, np.uint8)])
    tiles = np.random.default_rng(7).integers(0, 256, (H // 120, W // 240, 4), dtype=np.uint8)
    flat = np.ascontiguousarray(np.repeat(np.repeat(tiles, 120, axis=0), 240, axis=1))
    # ---- yardstick: k_convert_vec rgb8 -> rgba8 on n frames
    src = torch.from_numpy(photo.reshape(-1)).to(dev).repeat(n)
    dst = torch.empty(n * W * H * 4, dtype=torch.uint8, device=dev)
    ms, mn = timed(lambda: _capi.check(L.gamut_hip_scanlines_convert_device(O.PT["rgb8"], src.data_ptr(), W * 3, W * H * 3, O.PT["rgba8"], dst.data_ptr(), W * 4, W * H * 4,
                                                                            W, H, n, stream)), a.steps, a.warmup, torch.cuda.synchronize)
    yard = n * W * H * 7 / (ms * 1e-3) / 8e12
    emit(batch="yardstick k_convert_vec rgb8->rgba8", images=n, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(n * W * H / ms / 1e3, 1),
         roofline_fraction_algorithmic=round(yard, 4))
    del dst, src
    for name, px, rle in (("rgb8 photo-like", photo, 1), ("rgba8 photo-like", photo_a, 1), ("rgba8 flat", flat, 1), ("rgb8 photo-like, no run-length packets", photo, 0)):
        comp = px.shape[2]
        fb = W * H * comp
        want = tga_write_ref_c.encode(px, bool(rle))
        t = []
        for _ in range(6):                                              # the C restatement on one host core: 1 cold + 5 warm
            t0 = time.perf_counter(); tga_write_ref_c.encode(px, bool(rle)); t.append(time.perf_counter() - t0)
        host_ms = 1e3 * float(np.median(t[1:]))
        s = torch.from_numpy(px.reshape(-1)).to(dev).repeat(n)
        bound = L.gamut_hip_tga_encode_bound(W, H, comp)
        slot = (bound + 255) // 256 * 256
        out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
        ptrs = (C.c_void_p * n)(*[s.data_ptr() + i * fb for i in range(n)]); pitch = (C.c_int64 * n)(*([W * comp] * n))
        wa = (C.c_int32 * n)(*([W] * n)); ha = (C.c_int32 * n)(*([H] * n)); ca = (C.c_int32 * n)(*([comp] * n)); ra = (C.c_int32 * n)(*([rle] * n))
        offs = (C.c_int64 * n)(*[i * slot for i in range(n)]); lens = (C.c_int64 * n)(); st = (C.c_int * n)()
        run = lambda: _capi.check(L.gamut_hip_tga_encode_batch_device(ptrs, pitch, wa, ha, ca, ra, n, offs, out.data_ptr(), lens, st, stream))
        run()
        assert list(lens) == [len(want)] * n, "encode length"
        for i in (0, n - 1):
            assert out[i * slot:i * slot + len(want)].cpu().numpy().tobytes() == want, "encode parity"
        kms, stages = [], []
        for _ in range(a.warmup + a.steps):
            run()
            kms.append(L.gamut_hip_tga_last_encode_kernel_ms()); stages.append([L.gamut_hip_tga_last_encode_stage_ms(k) for k in range(3)])
        kms, stages = kms[a.warmup:], np.array(stages[a.warmup:])
        km = float(np.median(kms))
        sm = [float(x) for x in np.median(stages, axis=0)]
        ms, mn = timed(run, a.steps, a.warmup, torch.cuda.synchronize)
        bytes_once = n * (fb + len(want))
        emit(batch="encode " + name, images=n, kernel_ms=round(km, 3), kernel_ms_min=round(min(kms), 3), call_ms=round(ms, 3), call_ms_min=round(mn, 3),
             stage_ms=dict(rows=round(sm[0], 3), offsets=round(sm[1], 3), write=round(sm[2], 3)),
             stage_roofline_fraction=dict(rows=round(n * fb / (sm[0] * 1e-3) / 8e12, 4) if rle else None, write=round(bytes_once / (sm[2] * 1e-3) / 8e12, 4)),
             bytes_out=n * len(want), file_bytes=len(want), mpx_per_s=round(n * W * H / km / 1e3, 1),
             roofline_fraction_algorithmic=round(bytes_once / (km * 1e-3) / 8e12, 4), yardstick_fraction_same_run=round(yard, 4),
             host_one_core_ms_per_frame=round(host_ms, 3), host_one_core_mpx_per_s=round(W * H / host_ms / 1e3, 1))
        del out, s
    if a.json:
        with open(a.json, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
