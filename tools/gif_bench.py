"""GIF decode throughput (gamut_hip_gif_decode_batch_device), one JSON line per batch, appended to profiles/gif_bench.jsonl.

    python tools/gif_bench.py [--files 256] [--frames 16] [--distinct 2] [--steps 5] [--warmup 2] [--json profiles/gif_bench.jsonl]

A batch is `--files` files of 480 x 270 with `--frames` full-screen frames each, written by the tests' GIF writer (tests/gif_gen.py): once
photo-like content (short strings, the table fills and clears), once flat content (long strings).  The writer is Python, so `--distinct`
files are written and repeated to fill the batch; every frame is still decoded on its own.  Each batch is checked against the C
restatement of the reference (tests/c/gif_ref.c) -- every distinct file, every layer -- before it is timed.
With GAMUT_HIP_GIF_TIMING=1 (set here) the library brackets its two kernels with events once the files are resident in HBM:
`lzw_ms` (k_gif_lzw) and `compose_ms` (k_gif_compose).  `call_ms` is the whole call with host parsing, staging and PCIe inside;
`mpx_per_s` counts output pixels (layers x width x height) over the whole call, `kernel_mpx_per_s` over the two kernels.
For context: the restated reference on one host core and Pillow (every frame converted to RGBA) on the same files in this process."""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
W, H = 480, 270


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "gif_bench.jsonl"))
    a = ap.parse_args()
    os.environ["GAMUT_HIP_GIF_TIMING"] = "1"                           # read once by the library, at its first decode call
    import torch
    from PIL import Image, ImageSequence
    import gif_gen as g
    import gif_ref_c
    from gamut_amd import _capi
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    n, layer_px = a.files, W * H
    slot = a.frames * layer_px * 4
    pal = g.palette(256, 7)
    for content in ("photo-like", "flat"):
        rng = np.random.default_rng(len(content))
        distinct = []
        for d in range(a.distinct):
            frames = [g.frame(0, 0, W, H, g.photo_like(rng, W, H) if content == "photo-like" else np.roll(g.flat(W, H, 8, 16), 977 * (d * a.frames + k)), cs=8,
                              gce_bytes=g.gce(1, None, 4)) for k in range(a.frames)]
            distinct.append(g.make(W, H, frames, gct=pal))
        files = [distinct[i % a.distinct] for i in range(n)]
        bufs = [np.frombuffer(f, np.uint8) for f in distinct]
        ptrs = (C.c_void_p * n)(*[bufs[i % a.distinct].ctypes.data for i in range(n)])
        lens = (C.c_size_t * n)(*[len(f) for f in files])
        offs = (C.c_int64 * n)(*[i * slot for i in range(n)]); caps = (C.c_int64 * n)(*([slot] * n))
        out = torch.empty(n * slot, dtype=torch.uint8, device="cuda")
        st = (C.c_int * n)()
        run = lambda: _capi.check(L.gamut_hip_gif_decode_batch_device(ptrs, lens, n, offs, caps, out.data_ptr(), None, st, stream))
        run()
        refs, ref_ms = [], 0.0
        for f in distinct:                                                  # ONE gifref_load call (open + every frame) into a buffer that exists already
            fb = np.frombuffer(f + b"\0", np.uint8); ref = np.zeros((a.frames, H, W, 4), np.uint8)
            i4 = np.zeros(4, np.int32); f2 = np.zeros(2, np.float32)
            t0 = time.perf_counter()
            ok = gif_ref_c.lib().gifref_load(fb.ctypes.data, len(f), ref.ctypes.data, ref.size, i4.ctypes.data, f2.ctypes.data)
            ref_ms += 1e3 * (time.perf_counter() - t0) / a.distinct
            assert ok and tuple(i4[:3]) == (W, H, a.frames)
            refs.append(ref)
        for i in list(range(a.distinct)) + [n - 1]:
            assert np.array_equal(out[i * slot:(i + 1) * slot].cpu().numpy(), refs[i % a.distinct].reshape(-1)), ("parity", content, i)
        t0 = time.perf_counter()
        for f in distinct:
            for fr in ImageSequence.Iterator(Image.open(io.BytesIO(f))):
                fr.convert("RGBA")
        pil_ms = 1e3 * (time.perf_counter() - t0) / a.distinct
        call, lzw, comp = [], [], []
        for k in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); run(); call.append(1e3 * (time.perf_counter() - t0))     # (the call returns when the pixels are in place)
            lzw.append(L.gamut_hip_gif_last_kernel_ms(0)); comp.append(L.gamut_hip_gif_last_kernel_ms(1))
        call, lzw, comp = (np.array(x[a.warmup:]) for x in (call, lzw, comp))
        mpx = n * a.frames * layer_px / 1e6
        rows.append(json.dumps(dict(
            tool="gif_bench", content=content, files=n, frames_per_file=a.frames, width=W, height=H, distinct_files=a.distinct,
            file_bytes=int(np.mean([len(f) for f in distinct])), steps=a.steps, warmup=a.warmup,
            lzw_ms=round(float(np.median(lzw)), 3), lzw_ms_min=round(float(lzw.min()), 3),
            compose_ms=round(float(np.median(comp)), 3), compose_ms_min=round(float(comp.min()), 3),
            call_ms=round(float(np.median(call)), 3), call_ms_min=round(float(call.min()), 3),
            mpx_per_s=round(mpx / (float(np.median(call)) * 1e-3), 1), kernel_mpx_per_s=round(mpx / (float(np.median(lzw + comp)) * 1e-3), 1),
            compose_fraction_of_8TBps=round(n * slot / (float(np.median(comp)) * 1e-3) / 8e12, 4),
            reference_one_core_ms_per_file=round(ref_ms, 2), reference_one_core_mpx_per_s=round(a.frames * layer_px / 1e6 / (ref_ms * 1e-3), 1),
            pillow_ms_per_file=round(pil_ms, 2), pillow_mpx_per_s=round(a.frames * layer_px / 1e6 / (pil_ms * 1e-3), 1))))
        print(rows[-1], flush=True)
        del out
    if a.json:
        with open(a.json, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
