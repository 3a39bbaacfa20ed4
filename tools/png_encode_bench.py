"""PNG encode throughput and size: a batch of 1920x1080 frames already in HBM -> PNG files in HBM (gamut_hip_png_encode_batch_device).

    python tools/png_encode_bench.py [--images 1024] [--comp 4|3] [--content photo|flat] [--filter -1|0..4] [--level 0..10]
                                     [--steps 3] [--warmup 1] [--json out.jsonl]

Before timing, a few files of the batch are checked against the serial C restatement (tests/c/png_write_ref.c): container bytes, and
zlib.decompress(payload) == the restatement's filtered stream.  Reports ms per batch, Mpx/s, the fraction of 8 TB/s counted on
algorithmic traffic (frames read once + files written once), and the payload size of frame 0 against zlib level 1 and zlib's
Z_HUFFMAN_ONLY stream on the same filtered bytes.  Per-stage kernel times come from running this tool under
`rocprofv3 --kernel-trace --stats -- python tools/png_encode_bench.py ...` (the k_penc_* rows)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1920, 1080


def frames(kind, comp, n_distinct):
    from gamut_amd import synth
    out = []
    rng = np.random.default_rng(5)
    for s in range(n_distinct):
        if kind == "photo":
            px = np.ascontiguousarray(synth.photo_rgb(W, H, 100 + s))
        else:
            px = np.full((H, W, 3), 235, np.uint8)
            for _ in range(80):
                y, x = rng.integers(0, H - 8), rng.integers(0, W - 8)
                px[y: y + rng.integers(4, 300), x: x + rng.integers(4, 500)] = rng.integers(0, 256, 3)
        if comp == 4:
            px = np.dstack([px, np.full((H, W), 255, np.uint8)])
        out.append(np.ascontiguousarray(px))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--comp", type=int, choices=[3, 4], default=4)
    ap.add_argument("--content", choices=["photo", "flat"], default="photo")
    ap.add_argument("--filter", type=int, default=-1)
    ap.add_argument("--level", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch
    import png_write_ref_c as PW
    from gamut_amd import _capi
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    dev = torch.device("cuda", 0)
    host = frames(a.content, a.comp, a.distinct)
    fb = W * H * a.comp
    n = a.images
    src = torch.empty((n, fb), dtype=torch.uint8, device=dev)
    for k, f in enumerate(host):
        src[k] = torch.from_numpy(f.reshape(-1)).to(dev)
    for i in range(len(host), n):
        src[i] = src[i % len(host)]
    bound = L.gamut_hip_png_encode_bound(W, H, a.comp, 0)
    ptrs = (C.c_void_p * n)(*[src.data_ptr() + i * fb for i in range(n)])
    pitch = (C.c_int64 * n)(*([W * a.comp] * n))
    wa = (C.c_int * n)(*([W] * n)); ha = (C.c_int * n)(*([H] * n)); ca = (C.c_int * n)(*([a.comp] * n)); sa = (C.c_int * n)()
    fa = (C.c_int * n)(*([a.filter] * n)); la = (C.c_int * n)(*([a.level] * n))
    offs = (C.c_int64 * n)(*[i * bound for i in range(n)])
    out = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    lens = (C.c_int64 * n)(); status = (C.c_int * n)()
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        _capi.check(L.gamut_hip_png_encode_batch_device(ptrs, pitch, wa, ha, ca, sa, fa, la, n, offs, out.data_ptr(), lens, status, stream))

    run()                                                           # parity before timing
    sizes = {}
    for k in sorted({0, min(len(host), n) - 1, n - 1}):
        got = out[k * bound: k * bound + lens[k]].cpu().numpy().tobytes()
        px = host[k % len(host)]
        payload = PW.split(got)
        assert got == PW.file_around(W, H, a.comp, 0, payload), f"container mismatch on frame {k}"
        filt = PW.filt(px, a.filter)
        assert zlib.decompress(payload) == filt, f"filtered stream mismatch on frame {k}"
        if k == 0:
            co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
            sizes = dict(filtered_bytes=len(filt), payload_bytes=len(payload), zlib1_bytes=len(zlib.compress(filt, 1)),
                         zlib_huffman_only_bytes=len(co.compress(filt) + co.flush()))
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.steps):
        t0 = time.perf_counter(); run(); times.append(time.perf_counter() - t0)     # the call returns when the encode has finished
    ms = 1e3 * float(np.median(times))
    in_bytes = n * fb
    out_bytes = int(sum(lens[i] for i in range(n)))
    res = dict(tool="png_encode_bench", content=a.content, comp=a.comp, filter=a.filter, level=a.level, images=n, width=W, height=H,
               ms_per_batch=round(ms, 3), ms_min=round(1e3 * min(times), 3), mpx_per_s=round(n * W * H / ms / 1e3, 1),
               compression_ratio=round(in_bytes / out_bytes, 3), file_bytes=out_bytes,
               roofline_fraction_algorithmic=round((in_bytes + out_bytes) / (ms * 1e-3) / 8e12, 5),
               parity="C restatement: container bytes, inflate(payload) == filt", **sizes)
    if sizes:
        res["payload_over_zlib1"] = round(sizes["payload_bytes"] / sizes["zlib1_bytes"], 4)
        res["payload_over_huffman_only"] = round(sizes["payload_bytes"] / sizes["zlib_huffman_only_bytes"], 4)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
