"""TGA decode throughput (gamut_hip_tga_decode_batch_device), one JSON line per batch, appended to profiles/tga_bench.jsonl.

    python tools/tga_bench.py [--images 1024] [--decode-images 1024] [--steps 3] [--warmup 1] [--json profiles/tga_bench.jsonl]

Four 1920x1080 cases, each one file repeated: 24-bit unpacked, 8-bit indexed (24-bit colour map), 32-bit run-length photo-like (raw
packets of 128 pixels, what an encoder makes of noisy content) and 32-bit run-length flat (run packets of 128 pixels).  The library's
decode entry takes files in HOST memory; with GAMUT_HIP_TGA_TIMING=1 (set here) it brackets its kernels with events once the blob is
resident in HBM, and gamut_hip_tga_last_decode_kernel_ms() gives that time -- the "kernels" rows, with the fraction of 8 TB/s on
algorithmic bytes (file bytes + pixel bytes, each once).  The whole call, staging and PCIe inside, is reported separately
("file_level": true) and never as a roofline figure.  The yardstick is k_convert_vec rgb8 -> rgba8
(gamut_hip_scanlines_convert_device) on --images frames in the same process.  The C restatement (tests/c/tga_ref.c) is timed on one
host core per case, and every batch is checked against it on its last image before it is timed."""
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


def files(photo):
    """(name, file bytes, req_comp)"""
    import tga_gen
    rng = np.random.default_rng(1)
    bgr = np.ascontiguousarray(photo[::-1, :, ::-1])                        # bottom-up, B G R
    bgra = np.dstack([bgr, np.full((H, W), 255, np.uint8)])
    raw = np.concatenate([np.full((W * H // 128, 1), 127, np.uint8), bgra.reshape(-1, 512)], 1).tobytes()
    flat_px = np.repeat(rng.integers(0, 256, (H // 8, 1, 4), dtype=np.uint8), W * 8 // 128, 1).reshape(-1, 4)
    flat = np.concatenate([np.full((W * H // 128, 1), 0xFF, np.uint8), flat_px], 1).tobytes()
    idx = (photo[..., 1]).tobytes()                                          # the green channel as indices into a 256-entry colour map
    return [("24-bit unpacked -> rgb8", tga_gen.header(W, H, 2, 24) + bgr.tobytes(), 0),
            ("8-bit indexed, 24-bit colour map -> rgb8", tga_gen.header(W, H, 1, 8, 24, pal_len=256) + rng.integers(0, 256, 768, dtype=np.uint8).tobytes() + idx, 0),
            ("32-bit RLE photo-like (raw packets) -> rgba8", tga_gen.header(W, H, 10, 32, desc_extra=8) + raw, 0),
            ("32-bit RLE flat (run packets) -> rgba8", tga_gen.header(W, H, 10, 32, desc_extra=8) + flat, 0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--decode-images", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "tga_bench.jsonl"))
    a = ap.parse_args()
    os.environ["GAMUT_HIP_TGA_TIMING"] = "1"                           # read once by the library, at its first decode call
    import torch
    import oracle_lib as O
    import tga_ref_c
    from gamut_amd import _capi, synth
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(**kw):
        rows.append(json.dumps(dict(tool="tga_bench", width=W, height=H, **kw)))
        print(rows[-1], flush=True)

    photo = np.ascontiguousarray(synth.photo_rgb(W, H, 101))
    n = a.images
    # ---- yardstick: k_convert_vec rgb8 -> rgba8 on n frames
    src = torch.from_numpy(photo.reshape(-1)).to(dev).repeat(n)
    dst = torch.empty(n * W * H * 4, dtype=torch.uint8, device=dev)
    ms, mn = timed(lambda: _capi.check(L.gamut_hip_scanlines_convert_device(O.PT["rgb8"], src.data_ptr(), W * 3, W * H * 3, O.PT["rgba8"], dst.data_ptr(), W * 4, W * H * 4,
                                                                            W, H, n, stream)), a.steps, a.warmup, torch.cuda.synchronize)
    emit(batch="yardstick k_convert_vec rgb8->rgba8", images=n, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(n * W * H / ms / 1e3, 1),
         roofline_fraction_algorithmic=round(n * W * H * 7 / (ms * 1e-3) / 8e12, 4))
    del dst, src
    # ---- decode (files in host memory: the kernels with the blob resident, then the whole call with staging + PCIe inside)
    m = a.decode_images
    for name, f, req in files(photo):
        t0 = time.perf_counter(); ref = tga_ref_c.load(f, req); host_ms = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter(); ref = tga_ref_c.load(f, req); host_ms = min(host_ms, 1e3 * (time.perf_counter() - t0))
        comps = ref[0].shape[2]
        emit(batch="C restatement, one host core: " + name, images=1, ms_per_batch=round(host_ms, 3), mpx_per_s=round(W * H / host_ms / 1e3, 1), file_level=True)
        buf = np.frombuffer(f, np.uint8)
        ptrs = (C.c_void_p * m)(*([buf.ctypes.data] * m)); lens = (C.c_size_t * m)(*([buf.size] * m))
        ob = W * H * comps
        offs = (C.c_int64 * m)(*[i * ob for i in range(m)])
        out = torch.empty(m * ob, dtype=torch.uint8, device=dev)
        st = (C.c_int * m)()
        run = lambda: _capi.check(L.gamut_hip_tga_decode_batch_device(ptrs, lens, m, req, offs, out.data_ptr(), None, st, stream))
        run()
        assert np.array_equal(out[(m - 1) * ob:].cpu().numpy(), ref[0].reshape(-1)), "decode parity"
        kms = []
        for _ in range(a.warmup + a.steps):
            run(); kms.append(L.gamut_hip_tga_last_decode_kernel_ms())
        kms = kms[a.warmup:]
        km = float(np.median(kms))
        emit(batch="decode " + name + " (kernels, blob resident)", images=m, ms_per_batch=round(km, 3), ms_min=round(min(kms), 3), mpx_per_s=round(m * W * H / km / 1e3, 1),
             roofline_fraction_algorithmic=round(m * (len(f) + ob) / (km * 1e-3) / 8e12, 4), file_level=False, file_bytes=len(f))
        ms, mn = timed(run, a.steps, a.warmup, torch.cuda.synchronize)
        emit(batch="decode " + name, images=m, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(m * W * H / ms / 1e3, 1),
             file_level=True, file_bytes=len(f), gb_per_s_files=round(m * len(f) / (ms * 1e-3) / 1e9, 2))
        del out
    if a.json:
        with open(a.json, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
