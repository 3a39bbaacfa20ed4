"""SQZ encode throughput, one JSON line per measurement, appended to profiles/sqz_encode_bench.jsonl.

    python tools/sqz_encode_bench.py [--images 256] [--steps 5] [--warmup 2] [--json profiles/sqz_encode_bench.jsonl]

Workload: one 1920x1080 rgb8 frame repeated --images times, encoded as saveSQZ encodes (Oklab, 7 levels, snake scan, subsampling, the
default 2.5 bits per pixel), and the same frame as grey (same budget).  Reported, medians of --steps calls after --warmup:
  - the yardstick: k_convert_vec rgb8 -> rgba8 on the same pixel count in the same process;
  - the C restatement (tests/c/sqz_ref.c) on one host core: the whole encoder, and its forward steps alone (tests/c/sqz_ref_fwd.c);
  - the library's writer (gamut_hip_sqz_encode_coeffs) on one host core;
  - the front half alone (gamut_hip_sqz_analyze_batch_device, pixels and coefficients resident in HBM; GPU time between events on the
    stream, GAMUT_HIP_SQZ_TIMING=1), with its algorithmic HBM fraction: pixels read + coefficients written, each once, over time x 8 TB/s;
  - the decode back end (gamut_hip_sqz_reconstruct_batch_device) on the same geometry and the same coefficients: the natural comparison;
  - the whole call (gamut_hip_sqz_encode_batch_device): its three stages, wall time, bytes out.  Never a roofline figure: the writer
    is host code.
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
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "sqz_encode_bench.jsonl"))
    a = ap.parse_args()
    os.environ["GAMUT_HIP_SQZ_TIMING"] = "1"                           # read once by the library, at its first SQZ call
    import torch
    import oracle_lib as O
    import sqz_ref_c as R
    import sqz_ref_fwd_c as F
    from gamut_amd import _capi, synth
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(**kw):
        rows.append(json.dumps(dict(tool="sqz_encode_bench", width=W, height=H, **kw)))
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
    budget = L.gamut_hip_sqz_budget_from_flags(W, H, 0)
    grey = np.ascontiguousarray(photo[..., 1])
    for name, px, mode, ss in (("Oklab 2.5 bpp, 7 levels, snake, subsampled", photo, R.OKLAB, 1), ("grey, same budget, 7 levels, snake", grey, R.GREY, 0)):
        planes = 3 if mode else 1
        ob = W * H * planes
        # ---- host: the restatement on one core, whole and forward steps alone; the library's writer on one core
        ms, mn = med(lambda: R.encode(px, mode, 7, R.SNAKE, ss, budget), 3, 1)
        ref = R.encode(px, mode, 7, R.SNAKE, ss, budget)
        emit(batch="C restatement, one host core, whole encoder: " + name, images=1, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(W * H / ms / 1e3, 1), file_bytes=len(ref))
        ms, mn = med(lambda: F.analyze(px, mode, 7), 3, 1)
        emit(batch="C restatement, one host core, colour + DWT + sign-magnitude: " + name, images=1, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(W * H / ms / 1e3, 1))
        co_ref = F.analyze(px, mode, 7)
        d1 = _capi.SqzEncodeDesc(W, H, mode, 7, R.SNAKE, ss, budget)
        file1 = np.zeros(budget, np.uint8)
        n1 = C.c_int64(0)
        ms, mn = med(lambda: _capi.check(L.gamut_hip_sqz_encode_coeffs(co_ref.ctypes.data, C.byref(d1), file1.ctypes.data, C.byref(n1))), a.steps, a.warmup)
        assert file1[:n1.value].tobytes() == ref, "writer parity"
        writer_one = ms
        emit(batch="writer, one host core: " + name, images=1, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(W * H / ms / 1e3, 1), file_bytes=len(ref))
        # ---- the front half alone: pixels and coefficients resident
        dpx = torch.from_numpy(px.reshape(-1)).to(dev).repeat(n)
        dco = torch.empty(n * ob, dtype=torch.int16, device=dev)
        ptrs = (C.c_void_p * n)(*[dpx.data_ptr() + i * ob for i in range(n)])
        pitches = (C.c_int64 * n)(*([W * planes] * n))
        offs = (C.c_int64 * n)(*[i * ob for i in range(n)])
        descs = (_capi.SqzEncodeDesc * n)()
        for i in range(n):
            descs[i].width, descs[i].height, descs[i].color_mode, descs[i].levels, descs[i].scan_order, descs[i].subsampling, descs[i].budget = W, H, mode, 7, R.SNAKE, ss, budget
        st = (C.c_int * n)()
        ana = lambda: _capi.check(L.gamut_hip_sqz_analyze_batch_device(ptrs, pitches, descs, n, dco.data_ptr(), offs, st, stream))
        ana()
        assert np.array_equal(dco[(n - 1) * ob:].cpu().numpy(), co_ref), "analyze parity"
        km, kmin = med(ana, a.steps, a.warmup, lambda: L.gamut_hip_sqz_last_encode_stage_ms(0))
        emit(batch="front half alone (kernels, pixels and coefficients resident): " + name, images=n, ms_per_batch=round(km, 3), ms_min=round(kmin, 3),
             mpx_per_s=round(n * W * H / km / 1e3, 1), roofline_fraction_algorithmic=round(n * (ob + ob * 2) / (km * 1e-3) / 8e12, 4), launches=7, file_level=False)
        # ---- the decode back end on the same geometry and coefficients
        out = torch.empty(n * ob, dtype=torch.uint8, device=dev)
        rdescs = (_capi.SqzDesc * n)()
        for i in range(n):
            rdescs[i].width, rdescs[i].height, rdescs[i].color_mode, rdescs[i].levels, rdescs[i].coeff_offset = W, H, mode, 7, i * ob
        rec = lambda: _capi.check(L.gamut_hip_sqz_reconstruct_batch_device(dco.data_ptr(), rdescs, n, offs, out.data_ptr(), st, stream))
        rm, rmin = med(rec, a.steps, a.warmup, lambda: L.gamut_hip_sqz_last_decode_stage_ms(0))
        emit(batch="decode back end on the same coefficients (kernels): " + name, images=n, ms_per_batch=round(rm, 3), ms_min=round(rmin, 3), mpx_per_s=round(n * W * H / rm / 1e3, 1),
             roofline_fraction_algorithmic=round(n * (ob * 2 + ob) / (rm * 1e-3) / 8e12, 4), launches=7, forward_over_inverse=round(km / rm, 3))
        del out, dco
        # ---- the whole call: files in host memory
        files = np.zeros(n * budget, np.uint8)
        foffs = (C.c_int64 * n)(*[i * budget for i in range(n)])
        lens = (C.c_int64 * n)()
        run = lambda: _capi.check(L.gamut_hip_sqz_encode_batch_device(ptrs, pitches, descs, n, foffs, files.ctypes.data, lens, st, stream))
        run()
        assert files[(n - 1) * budget:(n - 1) * budget + lens[n - 1]].tobytes() == ref, "encode parity"
        ms, mn = med(run, a.steps, a.warmup)
        stages = []
        for _ in range(3):
            run(); stages.append([L.gamut_hip_sqz_last_encode_stage_ms(k) for k in range(3)])
        kern, writer, down = (float(np.median([s[k] for s in stages])) for k in range(3))
        bound = max((("front half kernels", kern), ("host writer", writer), ("download and staging", down)), key=lambda p: p[1])[0]
        emit(batch="whole encode call: " + name, images=n, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(n * W * H / ms / 1e3, 1), file_level=True,
             bytes_out=int(sum(lens)), kernels_ms=round(kern, 3), host_writer_pool_ms=round(writer, 3), download_staging_ms=round(down, 3), writer_share=round(writer / ms, 3),
             bounded_by=bound, host_threads=L.gamut_hip_host_threads(), writer_one_core_ms_per_file=round(writer_one, 3))
        del dpx, files
    if a.json:
        with open(a.json, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
