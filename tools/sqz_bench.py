"""SQZ decode throughput, one JSON line per measurement, appended to profiles/sqz_bench.jsonl.

    python tools/sqz_bench.py [--images 256] [--steps 5] [--warmup 2] [--json profiles/sqz_bench.jsonl]

Workload: one 1920x1080 frame as the plugin's saveSQZ writes it (Oklab, 7 levels, snake scan, subsampling, 2.5 bits per pixel), repeated
--images times, and the same frame as grey (same budget).  Reported, medians of --steps calls after --warmup:
  - the C restatement (tests/c/sqz_ref.c) on one host core, coefficient stage and pixel stage;
  - the library's front end (gamut_hip_sqz_decode_coeffs) on one host core, and on the pool inside the file-level call;
  - the back end alone (gamut_hip_sqz_reconstruct_batch_device, coefficients resident in HBM; GPU time between events on the stream,
    GAMUT_HIP_SQZ_TIMING=1), with its algorithmic HBM fraction: coefficients read + pixels written, each once, over time x 8 TB/s;
  - the whole file-level call (gamut_hip_sqz_decode_batch_device), host front end, staging and PCIe inside: never a roofline figure;
  - the yardstick: k_convert_vec rgb8 -> rgba8 on the same pixel count in the same process.
Every batch is checked against the restatement on its last image before it is timed."""
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


def med(run, steps, warmup, read=None):
    """median and minimum of run()'s wall milliseconds, or of read() after each run"""
    t = []
    for k in range(warmup + steps):
        t0 = time.perf_counter(); run(); wall = 1e3 * (time.perf_counter() - t0)
        if k >= warmup:
            t.append(wall if read is None else read())
    return float(np.median(t)), float(min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "sqz_bench.jsonl"))
    a = ap.parse_args()
    os.environ["GAMUT_HIP_SQZ_TIMING"] = "1"                           # read once by the library, at its first decode call
    import torch
    import oracle_lib as O
    import sqz_ref_c as R
    from gamut_amd import _capi, synth
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(**kw):
        rows.append(json.dumps(dict(tool="sqz_bench", width=W, height=H, **kw)))
        print(rows[-1], flush=True)

    def sync_wall(run):
        def f():
            run(); torch.cuda.synchronize()
        return f

    photo = np.ascontiguousarray(synth.photo_rgb(W, H, 101))
    n = a.images
    # ---- yardstick: k_convert_vec rgb8 -> rgba8 on n frames
    src = torch.from_numpy(photo.reshape(-1)).to(dev).repeat(n)
    dst = torch.empty(n * W * H * 4, dtype=torch.uint8, device=dev)
    ms, mn = med(sync_wall(lambda: _capi.check(L.gamut_hip_scanlines_convert_device(O.PT["rgb8"], src.data_ptr(), W * 3, W * H * 3, O.PT["rgba8"], dst.data_ptr(), W * 4,
                                                                                    W * H * 4, W, H, n, stream))), a.steps, a.warmup)
    emit(batch="yardstick k_convert_vec rgb8->rgba8", images=n, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(n * W * H / ms / 1e3, 1),
         roofline_fraction_algorithmic=round(n * W * H * 7 / (ms * 1e-3) / 8e12, 4))
    del dst, src
    budget = 6 + int(W * H * 2.5 / 8)                                  # saveSQZ: SQZ_HEADER_SIZE + w * h * bpp / 8, bpp = 0x50 / 32
    grey = np.ascontiguousarray(photo[..., 1])
    for name, f in (("Oklab 2.5 bpp, 7 levels, snake, subsampled", R.encode(photo, R.OKLAB, 7, R.SNAKE, 1, budget)),
                    ("grey, same budget, 7 levels, snake", R.encode(grey, R.GREY, 7, R.SNAKE, 0, budget))):
        planes = 3 if name.startswith("Oklab") else 1
        mode = R.OKLAB if planes == 3 else R.GREY
        ob = W * H * planes
        # ---- host: the restatement and the library's front end on one core
        ms, mn = med(lambda: R.coeffs(f), 3, 1)
        emit(batch="C restatement, one host core, coefficient stage: " + name, images=1, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(W * H / ms / 1e3, 1), file_bytes=len(f))
        co_ref = R.coeffs(f)[0]
        ms, mn = med(lambda: R.pixels(co_ref, W, H, mode, 7), 3, 1)
        emit(batch="C restatement, one host core, pixel stage: " + name, images=1, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(W * H / ms / 1e3, 1))
        ref = R.pixels(co_ref, W, H, mode, 7)
        buf = np.frombuffer(f, np.uint8)
        co = np.zeros(ob, np.int16)
        info = _capi.SqzInfo()
        ms, mn = med(lambda: _capi.check(L.gamut_hip_sqz_decode_coeffs(buf.ctypes.data, buf.size, co.ctypes.data, co.size, C.byref(info))), a.steps, a.warmup)
        assert np.array_equal(co, co_ref), "front end parity"
        front_one = ms
        emit(batch="front end, one host core: " + name, images=1, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(W * H / ms / 1e3, 1), file_bytes=len(f))
        # ---- the back end alone: coefficients resident
        out = torch.empty(n * ob, dtype=torch.uint8, device=dev)
        offs = (C.c_int64 * n)(*[i * ob for i in range(n)])
        dco = torch.from_numpy(co).to(dev).repeat(n)
        descs = (_capi.SqzDesc * n)()
        for i in range(n):
            descs[i].width, descs[i].height, descs[i].color_mode, descs[i].levels, descs[i].coeff_offset = W, H, mode, 7, i * ob
        st = (C.c_int * n)()
        rec = lambda: _capi.check(L.gamut_hip_sqz_reconstruct_batch_device(dco.data_ptr(), descs, n, offs, out.data_ptr(), st, stream))
        rec()
        assert np.array_equal(out[(n - 1) * ob:].cpu().numpy(), ref.reshape(-1)), "reconstruct parity"
        km, kmin = med(rec, a.steps, a.warmup, lambda: L.gamut_hip_sqz_last_decode_stage_ms(0))
        emit(batch="back end alone (kernels, coefficients resident): " + name, images=n, ms_per_batch=round(km, 3), ms_min=round(kmin, 3), mpx_per_s=round(n * W * H / km / 1e3, 1),
             roofline_fraction_algorithmic=round(n * (ob * 2 + ob) / (km * 1e-3) / 8e12, 4), launches=7, file_level=False)
        del dco
        # ---- the whole file-level call
        ptrs = (C.c_void_p * n)(*([buf.ctypes.data] * n)); lens = (C.c_size_t * n)(*([buf.size] * n))
        out.fill_(0)
        stages = []
        run = lambda: _capi.check(L.gamut_hip_sqz_decode_batch_device(ptrs, lens, n, offs, out.data_ptr(), None, st, stream))
        run()
        assert np.array_equal(out[(n - 1) * ob:].cpu().numpy(), ref.reshape(-1)), "decode parity"
        ms, mn = med(sync_wall(run), a.steps, a.warmup, None)
        for _ in range(3):
            run(); stages.append([L.gamut_hip_sqz_last_decode_stage_ms(k) for k in range(3)])
        kern, front, stage = (float(np.median([s[k] for s in stages])) for k in range(3))
        emit(batch="file-level decode: " + name, images=n, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(n * W * H / ms / 1e3, 1), file_level=True,
             file_bytes=len(f), front_end_pool_ms=round(front, 3), staging_upload_queue_ms=round(stage, 3), kernels_ms=round(kern, 3),
             front_end_share=round(front / ms, 3), host_threads=L.gamut_hip_host_threads(), front_end_one_core_ms_per_file=round(front_one, 3))
        del out
    if a.json:
        with open(a.json, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
