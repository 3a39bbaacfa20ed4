"""The SQZ device writer against the host writer, one JSON line per measurement, appended to profiles/sqz_write_bench.jsonl.

    python tools/sqz_write_bench.py [--images 256] [--steps 5] [--warmup 2] [--json profiles/sqz_write_bench.jsonl]

Workload: DESIGN.md 4.23's own -- one 1920x1080 rgb8 frame repeated --images times, encoded as saveSQZ encodes (Oklab, 7 levels, snake
scan, subsampling, the default 2.5 bits per pixel), and the same frame as grey (same budget) -- at --images images and at ONE image.
Reported, medians of --steps calls after --warmup, with the minimum and the maximum of the timed calls (the spread):
  - the writer's kernels alone (gamut_hip_sqz_write_batch_device on resident coefficients; GPU time between events on the stream,
    GAMUT_HIP_SQZ_TIMING=1) and its table building;
  - the whole gamut_hip_sqz_encode_batch_to_device call (pixels in HBM -> files in HBM), wall time;
  - the whole host-output call gamut_hip_sqz_encode_batch_device with the device writer, wall time;
  - IN THE SAME PROCESS the same host-output call with the host writer: the path before the device writer existed, and the comparison.
Every batch is checked against the C restatement (tests/c/sqz_ref.c) on its last image before it is timed."""
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
    """median, minimum and maximum of run()'s wall milliseconds, or of read() after each run"""
    t = []
    for k in range(warmup + steps):
        t0 = time.perf_counter(); run(); wall = 1e3 * (time.perf_counter() - t0)
        if k >= warmup:
            t.append(wall if read is None else read())
    return round(float(np.median(t)), 3), round(float(min(t)), 3), round(float(max(t)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "sqz_write_bench.jsonl"))
    a = ap.parse_args()
    os.environ["GAMUT_HIP_SQZ_TIMING"] = "1"                           # read once by the library, at its first SQZ call
    import torch
    import sqz_ref_c as R
    from gamut_amd import _capi, synth
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(**kw):
        rows.append(json.dumps(dict(tool="sqz_write_bench", width=W, height=H, **kw)))
        print(rows[-1], flush=True)

    photo = np.ascontiguousarray(synth.photo_rgb(W, H, 101))
    grey = np.ascontiguousarray(photo[..., 1])
    budget = L.gamut_hip_sqz_budget_from_flags(W, H, 0)
    initial = L.gamut_hip_sqz_set_writer(0)
    try:
        for name, px, mode, ss in (("Oklab 2.5 bpp, 7 levels, snake, subsampled", photo, R.OKLAB, 1), ("grey, same budget, 7 levels, snake", grey, R.GREY, 0)):
            planes = 3 if mode else 1
            ob = W * H * planes
            ref = R.encode(px, mode, 7, R.SNAKE, ss, budget)
            for n in sorted({a.images, 1}, reverse=True):
                dpx = torch.from_numpy(px.reshape(-1)).to(dev).repeat(n)
                dco = torch.empty(n * ob, dtype=torch.int16, device=dev)
                dfiles = torch.zeros(n * budget, dtype=torch.uint8, device=dev)
                ptrs = (C.c_void_p * n)(*[dpx.data_ptr() + i * ob for i in range(n)])
                pitches = (C.c_int64 * n)(*([W * planes] * n))
                offs = (C.c_int64 * n)(*[i * ob for i in range(n)])
                foffs = (C.c_int64 * n)(*[i * budget for i in range(n)])
                descs = (_capi.SqzEncodeDesc * n)()
                for i in range(n):
                    descs[i].width, descs[i].height, descs[i].color_mode, descs[i].levels, descs[i].scan_order, descs[i].subsampling, descs[i].budget = W, H, mode, 7, R.SNAKE, ss, budget
                st = (C.c_int * n)()
                lens = (C.c_int64 * n)()
                last = lambda buf: bytes(buf[(n - 1) * budget:(n - 1) * budget + lens[n - 1]])
                common = dict(images=n, mpx=round(n * W * H / 1e6, 1))
                # ---- the writer alone, coefficients resident
                _capi.check(L.gamut_hip_sqz_analyze_batch_device(ptrs, pitches, descs, n, dco.data_ptr(), offs, st, stream))
                write = lambda: _capi.check(L.gamut_hip_sqz_write_batch_device(dco.data_ptr(), offs, descs, n, foffs, dfiles.data_ptr(), lens, st, stream))
                write()
                assert last(dfiles.cpu().numpy()) == ref, "device writer parity"
                km = med(write, a.steps, a.warmup, lambda: L.gamut_hip_sqz_last_write_stage_ms(0))
                tm = med(write, a.steps, 0, lambda: L.gamut_hip_sqz_last_write_stage_ms(1))
                wm = med(write, a.steps, a.warmup)
                emit(batch="device writer alone (coefficients and files resident): " + name, kernels_ms=km[0], kernels_min=km[1], kernels_max=km[2], tables_ms=tm[0],
                     call_ms=wm[0], call_min=wm[1], call_max=wm[2], bytes_out=int(sum(lens)), mpx_per_s_kernels=round(n * W * H / km[0] / 1e3, 1), **common)
                del dco
                # ---- pixels in HBM -> files in HBM
                to_dev = lambda: _capi.check(L.gamut_hip_sqz_encode_batch_to_device(ptrs, pitches, descs, n, foffs, dfiles.data_ptr(), lens, st, stream))
                dfiles.zero_()
                to_dev()
                assert last(dfiles.cpu().numpy()) == ref, "encode_batch_to_device parity"
                dm = med(to_dev, a.steps, a.warmup)
                emit(batch="whole call, files left in HBM (encode_batch_to_device): " + name, ms_per_batch=dm[0], ms_min=dm[1], ms_max=dm[2],
                     mpx_per_s=round(n * W * H / dm[0] / 1e3, 1), file_level=True, **common)
                del dfiles
                # ---- the host-output call with each writer, same process
                files = np.zeros(n * budget, np.uint8)
                run = lambda: _capi.check(L.gamut_hip_sqz_encode_batch_device(ptrs, pitches, descs, n, foffs, files.ctypes.data, lens, st, stream))
                res = {}
                for which, label in ((1, "device"), (0, "host")):
                    L.gamut_hip_sqz_set_writer(which)
                    files[:] = 0
                    run()
                    assert last(files) == ref, label + " writer parity"
                    res[label] = med(run, a.steps, a.warmup)
                    emit(batch="whole call, files to host memory (encode_batch_device), %s writer: %s" % (label, name), ms_per_batch=res[label][0], ms_min=res[label][1],
                         ms_max=res[label][2], mpx_per_s=round(n * W * H / res[label][0] / 1e3, 1), file_level=True, host_threads=L.gamut_hip_host_threads(), **common)
                L.gamut_hip_sqz_set_writer(0)
                emit(batch="host writer over device writer, host-output call: " + name, ratio=round(res["host"][0] / res["device"][0], 2),
                     device_faster_beyond_spread=bool(res["device"][2] < res["host"][1]), **common)
                del dpx, files
    finally:
        L.gamut_hip_sqz_set_writer(initial)
    if a.json:
        with open(a.json, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
