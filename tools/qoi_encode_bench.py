"""QOI encode throughput: a batch of 1920x1080 rgba8 frames already in HBM -> QOI streams in HBM (gamut_hip_qoi_encode_batch_device).

    python tools/qoi_encode_bench.py [--images 1024] [--content photo|flat] [--steps 5] [--warmup 2] [--cpu-threads 16] [--json out.json]

Before timing, a few frames of the batch are checked byte for byte against Pillow's QOI writer (payload) and the spec header.  Reports
ms per batch, Mpx/s, the compression ratio and the fraction of 8 TB/s counted on algorithmic traffic (frames read once + streams
written once; the kernels read the frames three times).  CPU context: Pillow's QOI writer on --cpu-threads host threads."""
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

W, H = 1920, 1080


def frames(kind, n_distinct):
    from gamut_amd import synth
    out = []
    rng = np.random.default_rng(5)
    for s in range(n_distinct):
        if kind == "photo":
            rgb = synth.photo_rgb(W, H, 100 + s)
            a = np.full((H, W, 1), 255, np.uint8)
            a[H // 3: H // 2, :, 0] = np.linspace(0, 255, W).astype(np.uint8)
            out.append(np.ascontiguousarray(np.concatenate([rgb, a], 2)))
        else:
            px = np.full((H, W, 4), 235, np.uint8); px[..., 3] = 255
            for _ in range(80):
                y, x = rng.integers(0, H - 8), rng.integers(0, W - 8)
                px[y: y + rng.integers(4, 300), x: x + rng.integers(4, 500)] = (*rng.integers(0, 256, 3), 255)
            out.append(px)
    return out


def pillow_qoi(px):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(px, "RGBA").save(b, format="QOI")
    return b.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--content", choices=["photo", "flat"], default="photo")
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-images", type=int, default=64)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch
    from gamut_amd import _capi
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    dev = torch.device("cuda", 0)
    host = frames(a.content, a.distinct)
    fb = W * H * 4
    src = torch.empty((a.images, fb), dtype=torch.uint8, device=dev)
    for k, f in enumerate(host):
        src[k] = torch.from_numpy(f.reshape(-1)).to(dev)
    for i in range(len(host), a.images):
        src[i] = src[i % len(host)]
    d = _capi.QoiDesc(); d.width, d.height, d.channels, d.colorspace = W, H, 4, 0
    bound = L.gamut_hip_qoi_encode_bound(C.byref(d))
    n = a.images
    descs = (_capi.QoiDesc * n)(*([d] * n))
    ptrs = (C.c_void_p * n)(*[src.data_ptr() + i * fb for i in range(n)])
    pitch = (C.c_int64 * n)(*([W * 4] * n))
    offs = (C.c_int64 * n)(*[i * bound for i in range(n)])
    out = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    lens = (C.c_int64 * n)(); status = (C.c_int * n)()
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        _capi.check(L.gamut_hip_qoi_encode_batch_device(ptrs, pitch, descs, n, offs, out.data_ptr(), lens, status, stream))

    run()                                                           # parity before timing
    for k in sorted({0, len(host) - 1, n - 1}):
        got = out[k * bound: k * bound + lens[k]].cpu().numpy().tobytes()
        exp = pillow_qoi(host[k % len(host)])
        assert got[:14] == b"qoif" + W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([4, 0]) and got[14:] == exp[14:], f"parity failure on frame {k}"
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.steps):
        t0 = time.perf_counter(); run(); times.append(time.perf_counter() - t0)     # the call returns when the encode has finished
    ms = 1e3 * float(np.median(times))
    in_bytes = n * fb
    out_bytes = int(sum(lens[i] for i in range(n)))
    res = dict(tool="qoi_encode_bench", content=a.content, images=n, width=W, height=H, ms_per_batch=round(ms, 3),
               ms_min=round(1e3 * min(times), 3), mpx_per_s=round(n * W * H / ms / 1e3, 1),
               compression_ratio=round(in_bytes / out_bytes, 3), stream_bytes=out_bytes,
               roofline_fraction_algorithmic=round((in_bytes + out_bytes) / (ms * 1e-3) / 8e12, 4), parity="pillow payload + spec header")
    # CPU context: Pillow's writer on host threads
    cpu_n = min(a.cpu_images, n)
    t0 = time.perf_counter()
    with cf.ThreadPoolExecutor(a.cpu_threads) as ex:
        list(ex.map(lambda k: pillow_qoi(host[k % len(host)]), range(cpu_n)))
    cpu_s = time.perf_counter() - t0
    res.update(cpu_threads=a.cpu_threads, cpu_cores_visible=len(os.sched_getaffinity(0)), cpu_images=cpu_n,
               cpu_ms_per_batch_extrapolated=round(1e3 * cpu_s * n / cpu_n, 1), cpu_mpx_per_s=round(cpu_n * W * H / cpu_s / 1e6, 1))
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
