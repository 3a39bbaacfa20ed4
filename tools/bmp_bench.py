"""BMP decode / encode throughput (gamut_hip_bmp_*), one JSON line per batch, appended to profiles/bmp_bench.jsonl.

    python tools/bmp_bench.py [--images 1024] [--decode-images 128] [--steps 3] [--warmup 1] [--json profiles/bmp_bench.jsonl]

Encode: 1920x1080 frames resident in HBM -> files in HBM (rgba8 -> 32-bit, rgb8 -> 24-bit); the fraction of 8 TB/s is counted on
algorithmic bytes (pixel bytes + file bytes, each once).  Decode: the library's decode entry takes files in HOST memory; with
GAMUT_HIP_BMP_TIMING=1 (set here) it brackets its kernels with events once the blob is resident in HBM, and
gamut_hip_bmp_last_decode_kernel_ms() gives that time -- the "kernels" rows, with the roofline fraction.  The whole call, staging
and PCIe inside, is reported separately ("file_level": true) and never as a roofline figure.  The yardstick is
k_convert_vec rgb8 -> rgba8 (gamut_hip_scanlines_convert_device) on the same pixel count in the same process.  Every batch is checked
against the C restatement (tests/c/bmp_ref.c) on its first image before it is timed."""
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
    ap.add_argument("--decode-images", type=int, default=128)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "bmp_bench.jsonl"))
    a = ap.parse_args()
    os.environ["GAMUT_HIP_BMP_TIMING"] = "1"                           # read once by the library, at its first decode call
    import torch
    import bmp_gen
    import bmp_ref_c
    import oracle_lib as O
    from gamut_amd import _capi, synth
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(**kw):
        rows.append(json.dumps(dict(tool="bmp_bench", width=W, height=H, **kw)))
        print(rows[-1], flush=True)

    photo = np.ascontiguousarray(synth.photo_rgb(W, H, 101))
    rgba = np.dstack([photo, np.full((H, W), 255, np.uint8)])
    n = a.images
    # ---- yardstick: k_convert_vec rgb8 -> rgba8 on n frames
    src = torch.from_numpy(photo.reshape(-1)).to(dev).repeat(n)
    dst = torch.empty(n * W * H * 4, dtype=torch.uint8, device=dev)
    ms, mn = timed(lambda: _capi.check(L.gamut_hip_scanlines_convert_device(O.PT["rgb8"], src.data_ptr(), W * 3, W * H * 3, O.PT["rgba8"], dst.data_ptr(), W * 4, W * H * 4,
                                                                            W, H, n, stream)), a.steps, a.warmup, torch.cuda.synchronize)
    emit(batch="yardstick k_convert_vec rgb8->rgba8", images=n, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(n * W * H / ms / 1e3, 1),
         roofline_fraction_algorithmic=round(n * W * H * 7 / (ms * 1e-3) / 8e12, 4))
    del dst
    # ---- encode, inputs resident in HBM
    for comp, px in ((4, rgba), (3, photo)):
        fb = W * H * comp
        s = src if comp == 3 else torch.from_numpy(px.reshape(-1)).to(dev).repeat(n)
        bound = L.gamut_hip_bmp_encode_bound(W, H, comp)
        slot = (bound + 255) // 256 * 256
        out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
        ptrs = (C.c_void_p * n)(*[s.data_ptr() + i * fb for i in range(n)]); pitch = (C.c_int64 * n)(*([W * comp] * n))
        wa = (C.c_int32 * n)(*([W] * n)); ha = (C.c_int32 * n)(*([H] * n)); ca = (C.c_int32 * n)(*([comp] * n))
        offs = (C.c_int64 * n)(*[i * slot for i in range(n)]); lens = (C.c_int64 * n)(); st = (C.c_int * n)()
        run = lambda: _capi.check(L.gamut_hip_bmp_encode_batch_device(ptrs, pitch, wa, ha, ca, None, None, n, offs, out.data_ptr(), lens, st, stream))
        run()
        assert out[:bound].cpu().numpy().tobytes() == bmp_ref_c.write(px), "encode parity"
        ms, mn = timed(run, a.steps, a.warmup, torch.cuda.synchronize)
        emit(batch=f"encode {'rgba8 -> 32-bit' if comp == 4 else 'rgb8 -> 24-bit'} file", images=n, ms_per_batch=round(ms, 3), ms_min=round(mn, 3),
             mpx_per_s=round(n * W * H / ms / 1e3, 1), roofline_fraction_algorithmic=round(n * (fb + bound) / (ms * 1e-3) / 8e12, 4), file_level=False)
        del out, s
    del src
    # ---- decode, file-level (files in host memory: staging + PCIe inside)
    m = a.decode_images
    zero_a = np.random.default_rng(1).integers(0, 256, (H, W, 4), dtype=np.uint8); zero_a[..., 3] = 0
    some_a = zero_a.copy(); some_a[0, 0, 3] = 1
    cases = [("24-bit -> rgba8", bmp_gen.make(W, H, 24, 40, seed=1), 4), ("24-bit -> rgb8", bmp_gen.make(W, H, 24, 40, seed=1), 3),
             ("8-bit palette -> rgba8", bmp_gen.make(W, H, 8, 40, seed=2), 4),
             ("32-bit BI_RGB -> rgba8, all_a rewrite fires", bmp_gen.make(W, H, 32, 40, body=zero_a.tobytes()), 4),
             ("32-bit BI_RGB -> rgba8, no rewrite", bmp_gen.make(W, H, 32, 40, body=some_a.tobytes()), 4)]
    for name, f, req in cases:
        buf = np.frombuffer(f, np.uint8)
        ptrs = (C.c_void_p * m)(*([buf.ctypes.data] * m)); lens = (C.c_size_t * m)(*([buf.size] * m))
        ob = W * H * req
        offs = (C.c_int64 * m)(*[i * ob for i in range(m)])
        out = torch.empty(m * ob, dtype=torch.uint8, device=dev)
        st = (C.c_int * m)()
        run = lambda: _capi.check(L.gamut_hip_bmp_decode_batch_device(ptrs, lens, m, req, offs, out.data_ptr(), None, st, stream))
        run()
        assert np.array_equal(out[(m - 1) * ob:].cpu().numpy(), bmp_ref_c.load(f, req)[0].reshape(-1)), "decode parity"
        kms = []
        for _ in range(a.warmup + a.steps):
            run(); kms.append(L.gamut_hip_bmp_last_decode_kernel_ms())
        kms = kms[a.warmup:]
        km = float(np.median(kms))
        emit(batch="decode " + name + " (kernels, blob resident)", images=m, ms_per_batch=round(km, 3), ms_min=round(min(kms), 3), mpx_per_s=round(m * W * H / km / 1e3, 1),
             roofline_fraction_algorithmic=round(m * (len(f) + ob) / (km * 1e-3) / 8e12, 4), file_level=False)
        ms, mn = timed(run, a.steps, a.warmup, torch.cuda.synchronize)
        emit(batch="decode " + name, images=m, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(m * W * H / ms / 1e3, 1),
             file_level=True, file_bytes=len(f), gb_per_s_files=round(m * len(f) / (ms * 1e-3) / 1e9, 2))
        del out
    if a.json:
        with open(a.json, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
