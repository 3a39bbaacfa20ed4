"""SQZ read on the device against the host front end, one JSON line per measurement, appended to profiles/sqz_read_bench.jsonl.

    python tools/sqz_read_bench.py [--images 256,1] [--steps 5] [--warmup 2] [--json profiles/sqz_read_bench.jsonl]

Workload: tools/sqz_bench.py's -- one 1920x1080 frame as the plugin's saveSQZ writes it (Oklab, 7 levels, snake scan, subsampling,
2.5 bits per pixel) repeated --images times, and the same frame as grey (same budget).  Reported per batch size, medians of --steps
calls after --warmup, all in ONE process, with the minimum and the spread (max - min) of the calls:
  - the reader's kernels alone (gamut_hip_sqz_read_batch_device; GPU time between events, GAMUT_HIP_SQZ_TIMING=1) and the wall clock
    of that call (table building, staging and upload of the files inside);
  - the file-level call (gamut_hip_sqz_decode_batch_device) with the device reader;
  - the same call with the host reader.
The coefficients and the pixels of the last image of every batch are checked against the C restatement (tests/c/sqz_ref.c) before
anything is timed.  The last line per batch states whether the device path beats the host path by more than the spread of the calls."""
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


def series(run, steps, warmup, read=None):
    """run()'s wall milliseconds (or read() after each run) -> median, minimum, spread"""
    t = []
    for k in range(warmup + steps):
        t0 = time.perf_counter(); run(); wall = 1e3 * (time.perf_counter() - t0)
        if k >= warmup:
            t.append(wall if read is None else read())
    return float(np.median(t)), float(min(t)), float(max(t) - min(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", default="256,1")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "sqz_read_bench.jsonl"))
    a = ap.parse_args()
    os.environ["GAMUT_HIP_SQZ_TIMING"] = "1"                           # read once by the library, at its first call
    import torch
    import sqz_ref_c as R
    from gamut_amd import _capi, synth
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(**kw):
        rows.append(json.dumps(dict(tool="sqz_read_bench", width=W, height=H, **kw)))
        print(rows[-1], flush=True)

    photo = np.ascontiguousarray(synth.photo_rgb(W, H, 101))
    budget = 6 + int(W * H * 2.5 / 8)
    grey = np.ascontiguousarray(photo[..., 1])
    initial = L.gamut_hip_sqz_set_reader(0)
    try:
        for name, f in (("Oklab 2.5 bpp, 7 levels, snake, subsampled", R.encode(photo, R.OKLAB, 7, R.SNAKE, 1, budget)),
                        ("grey, same budget, 7 levels, snake", R.encode(grey, R.GREY, 7, R.SNAKE, 0, budget))):
            planes = 3 if name.startswith("Oklab") else 1
            mode = R.OKLAB if planes == 3 else R.GREY
            ob = W * H * planes
            co_ref = R.coeffs(f)[0]
            px_ref = R.pixels(co_ref, W, H, mode, 7).reshape(-1)
            buf = np.frombuffer(f, np.uint8)
            for n in [int(x) for x in a.images.split(",")]:
                ptrs = (C.c_void_p * n)(*([buf.ctypes.data] * n)); lens = (C.c_size_t * n)(*([buf.size] * n))
                offs = (C.c_int64 * n)(*[i * ob for i in range(n)])
                st = (C.c_int * n)()
                # ---- the reader alone
                dco = torch.empty(n * ob, dtype=torch.int16, device=dev)
                read = lambda: _capi.check(L.gamut_hip_sqz_read_batch_device(ptrs, lens, n, dco.data_ptr(), offs, None, st, stream))
                read()
                assert np.array_equal(dco[(n - 1) * ob:].cpu().numpy(), co_ref), "reader parity"
                km, kmin, ksp = series(read, a.steps, a.warmup, lambda: L.gamut_hip_sqz_last_read_stage_ms(0))
                wm, wmin, wsp = series(read, a.steps, a.warmup)
                tab = L.gamut_hip_sqz_last_read_stage_ms(1)
                emit(batch="reader alone: " + name, images=n, kernels_ms=round(km, 3), kernels_ms_min=round(kmin, 3), kernels_ms_spread=round(ksp, 3), call_ms=round(wm, 3),
                     call_ms_min=round(wmin, 3), call_ms_spread=round(wsp, 3), tables_staging_ms=round(tab, 3), file_bytes=len(f), mpx_per_s_kernels=round(n * W * H / km / 1e3, 1))
                del dco
                # ---- the file-level call, both readers
                out = torch.empty(n * ob, dtype=torch.uint8, device=dev)
                run = lambda: (_capi.check(L.gamut_hip_sqz_decode_batch_device(ptrs, lens, n, offs, out.data_ptr(), None, st, stream)), torch.cuda.synchronize())
                res = {}
                for which, label in ((1, "device"), (0, "host")):
                    L.gamut_hip_sqz_set_reader(which)
                    out.fill_(0)
                    run()
                    assert np.array_equal(out[(n - 1) * ob:].cpu().numpy(), px_ref), "decode parity, %s reader" % label
                    ms, mn, sp = series(run, a.steps, a.warmup)
                    res[label] = (ms, mn, sp)
                    emit(batch="file-level decode, %s reader: %s" % (label, name), images=n, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), ms_spread=round(sp, 3),
                         mpx_per_s=round(n * W * H / ms / 1e3, 1), back_end_kernels_ms=round(L.gamut_hip_sqz_last_decode_stage_ms(0), 3),
                         reader_kernels_ms=round(L.gamut_hip_sqz_last_read_stage_ms(0), 3) if which else None, host_threads=L.gamut_hip_host_threads())
                L.gamut_hip_sqz_set_reader(0)
                gain = res["host"][0] - res["device"][0]
                emit(batch="verdict: " + name, images=n, host_minus_device_ms=round(gain, 3), larger_spread_ms=round(max(res["host"][2], res["device"][2]), 3),
                     device_beats_host_by_more_than_the_spread=bool(gain > max(res["host"][2], res["device"][2])))
                del out
    finally:
        L.gamut_hip_sqz_set_reader(initial)
    if a.json:
        with open(a.json, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
