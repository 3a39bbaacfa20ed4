"""JPEG encode throughput: a batch of 1920x1080 rgb8 frames already in HBM -> baseline JPEG streams in HBM
(gamut_hip_jpeg_encode_batch_device).

    python tools/jpeg_encode_bench.py [--images 1024] [--content photo|flat] [--quality 90|95] [--steps 5] [--warmup 2]
                                      [--cpu-threads 16] [--json out.json]

Before timing, a few frames of the batch are checked byte for byte against the serial C restatement (tests/c/jpeg_write_ref.c).
Reports ms per batch, Mpx/s, the compression ratio and the fraction of 8 TB/s counted on algorithmic traffic (frames read once +
streams written once).  CPU context: the C restatement on --cpu-threads host threads, and Pillow's libjpeg encoder at the same
quality (a different encoder: its bytes differ)."""
import argparse
import concurrent.futures as cf
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

W, H = 1920, 1080


def frames(kind, n_distinct):
    from gamut_amd import synth
    out = []
    rng = np.random.default_rng(5)
    for s in range(n_distinct):
        if kind == "photo":
            out.append(np.ascontiguousarray(synth.photo_rgb(W, H, 100 + s)))
        else:
            px = np.full((H, W, 3), 235, np.uint8)
            for _ in range(80):
                y, x = rng.integers(0, H - 8), rng.integers(0, W - 8)
                px[y: y + rng.integers(4, 300), x: x + rng.integers(4, 500)] = rng.integers(0, 256, 3)
            out.append(px)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--content", choices=["photo", "flat"], default="photo")
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-images", type=int, default=64)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch
    import jpeg_write_ref_c as JW
    from gamut_amd import _capi
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    dev = torch.device("cuda", 0)
    host = frames(a.content, a.distinct)
    fb = W * H * 3
    src = torch.empty((a.images, fb), dtype=torch.uint8, device=dev)
    for k, f in enumerate(host):
        src[k] = torch.from_numpy(f.reshape(-1)).to(dev)
    for i in range(len(host), a.images):
        src[i] = src[i % len(host)]
    bound = L.gamut_hip_jpeg_encode_bound(W, H, 3, a.quality)
    n = a.images
    ptrs = (C.c_void_p * n)(*[src.data_ptr() + i * fb for i in range(n)])
    pitch = (C.c_int64 * n)(*([W * 3] * n))
    wa = (C.c_int * n)(*([W] * n)); ha = (C.c_int * n)(*([H] * n)); ca = (C.c_int * n)(*([3] * n)); qa = (C.c_int * n)(*([a.quality] * n))
    offs = (C.c_int64 * n)(*[i * bound for i in range(n)])
    out = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    lens = (C.c_int64 * n)(); status = (C.c_int * n)()
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        _capi.check(L.gamut_hip_jpeg_encode_batch_device(ptrs, pitch, wa, ha, ca, qa, n, offs, out.data_ptr(), lens, status, stream))

    run()                                                           # parity before timing
    for k in sorted({0, len(host) - 1, n - 1}):
        got = out[k * bound: k * bound + lens[k]].cpu().numpy().tobytes()
        assert got == JW.encode(host[k % len(host)], a.quality), f"parity failure on frame {k}"
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.steps):
        t0 = time.perf_counter(); run(); times.append(time.perf_counter() - t0)     # the call returns when the encode has finished
    ms = 1e3 * float(np.median(times))
    in_bytes = n * fb
    out_bytes = int(sum(lens[i] for i in range(n)))
    res = dict(tool="jpeg_encode_bench", content=a.content, quality=a.quality, images=n, width=W, height=H, ms_per_batch=round(ms, 3),
               ms_min=round(1e3 * min(times), 3), mpx_per_s=round(n * W * H / ms / 1e3, 1),
               compression_ratio=round(in_bytes / out_bytes, 3), stream_bytes=out_bytes,
               roofline_fraction_algorithmic=round((in_bytes + out_bytes) / (ms * 1e-3) / 8e12, 4), parity="C restatement, byte for byte")
    # CPU context: the serial C restatement (the same bytes) and Pillow's libjpeg (different bytes) on host threads
    cpu_n = min(a.cpu_images, n)
    for name, fn in (("cpu_ref", lambda k: JW.encode(host[k % len(host)], a.quality)), ("pillow", lambda k: _pillow(host[k % len(host)], a.quality))):
        t0 = time.perf_counter()
        with cf.ThreadPoolExecutor(a.cpu_threads) as ex:
            list(ex.map(fn, range(cpu_n)))
        cpu_s = time.perf_counter() - t0
        res[name + "_ms_per_batch_extrapolated"] = round(1e3 * cpu_s * n / cpu_n, 1)
        res[name + "_mpx_per_s"] = round(cpu_n * W * H / cpu_s / 1e6, 1)
    res.update(cpu_threads=a.cpu_threads, cpu_cores_visible=len(os.sched_getaffinity(0)), cpu_images=cpu_n)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "a") as f:
            f.write(line + "\n")


def _pillow(px, q):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(px, "RGB").save(b, format="JPEG", quality=q, subsampling=2 if q <= 90 else 0)
    return b.getvalue()


if __name__ == "__main__":
    main()
