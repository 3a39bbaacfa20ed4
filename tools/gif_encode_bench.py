"""GIF encode throughput (gamut_hip_gif_encode_batch_device), one JSON line per batch, appended to profiles/gif_encode_bench.jsonl.

    python tools/gif_encode_bench.py [--files 256] [--frames 16] [--distinct 2] [--steps 5] [--warmup 2] [--ref-repeats 5] [--json profiles/gif_encode_bench.jsonl]

A batch is `--files` animations of `--frames` rgba8 frames of 480 x 270 resident in HBM (the decode bench's shape): once photo-like
content (smooth fields plus noise, drifting from frame to frame), once flat content (a few colours in large areas).  `--distinct`
animations are generated and repeated to fill the batch (the sources are only read); every animation is still encoded on its own, into
its own slot.  Each batch is checked byte for byte against the C restatement of the reference (tests/c/gif_encode_ref.c) -- every distinct
animation and the last slot -- before it is timed: an untimed first call, `--warmup` discarded calls, then `--steps` timed ones.
With GAMUT_HIP_GIF_TIMING=1 (set here) the library brackets its five kernels with events: census_ms, plan_ms, lzw_ms, offsets_ms,
gather_ms.  `call_ms` is the whole call (tables, launches, the wait); `mpx_per_s` counts input pixels over the whole call.
The yardstick, in the same run: the C reference on one host core, per animation -- compiled and run once untimed, then the median of
`--ref-repeats` encodes of each distinct animation (`reference_16_cores_ms_per_batch` is that figure x files / 16)."""
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
W, H = 480, 270


def flat(frames, seed):
    rng = np.random.default_rng(seed)
    out = np.zeros((frames, H, W, 4), np.uint8)
    out[..., 3] = 255
    cols = rng.integers(0, 256, (8, 3), dtype=np.uint8)
    for f in range(frames):
        for k in range(8):
            x0, y0 = (k * 61 + 13 * f) % W, (k * 37 + 7 * f) % H
            out[f, y0:y0 + 90, x0:x0 + 160, :3] = cols[k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--distinct", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ref-repeats", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "gif_encode_bench.jsonl"))
    a = ap.parse_args()
    os.environ["GAMUT_HIP_GIF_TIMING"] = "1"                           # read once by the library, at its first encode call
    import torch
    import gif_encode_cases as cases
    import gif_encode_ref_c as ref_c
    from gamut_amd import _capi
    ref_c.lib()                                                         # compile the C reference now, outside every timed stretch
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    stream = torch.cuda.current_stream().cuda_stream
    n = a.files
    bound = ref_c.bound(W, H, a.frames)
    rows = []
    for content in ("photo-like", "flat"):
        distinct = [cases.photo_like(W, H, a.frames, seed=20 + d) if content == "photo-like" else flat(a.frames, 30 + d) for d in range(a.distinct)]
        refs, ref_ms = [], 0.0
        for px in distinct:                                                 # the yardstick: median of `--ref-repeats` encodes after one untimed encode
            refs.append(ref_c.encode(px)[0])
            t = []
            for _ in range(a.ref_repeats):
                t0 = time.perf_counter()
                ref_c.encode(px)
                t.append(1e3 * (time.perf_counter() - t0))
            ref_ms += float(np.median(t)) / a.distinct
        dev = [torch.from_numpy(px.reshape(-1)).cuda() for px in distinct]
        i32 = lambda v: (C.c_int32 * n)(*([v] * n))
        i64 = lambda v: (C.c_int64 * n)(*([v] * n))
        src = (C.c_void_p * n)(*[dev[i % a.distinct].data_ptr() for i in range(n)])
        offs = (C.c_int64 * n)(*[i * bound for i in range(n)])
        out = torch.empty(n * bound, dtype=torch.uint8, device="cuda")
        olen = (C.c_int64 * n)(); st = (C.c_int * n)()
        run = lambda: _capi.check(L.gamut_hip_gif_encode_batch_device(src, i64(W * 4), i64(W * H * 4), i32(W), i32(H), i32(a.frames), None, None, None, n,
                                                                      offs, out.data_ptr(), olen, st, stream))
        run()                                                               # untimed: allocations, code load
        for i in list(range(a.distinct)) + [n - 1]:
            r = refs[i % a.distinct]
            assert olen[i] == len(r) and out[i * bound:i * bound + len(r)].cpu().numpy().tobytes() == r, ("parity", content, i)
        call, ker = [], []
        for k in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); run(); call.append(1e3 * (time.perf_counter() - t0))     # (the call returns when the files are in place)
            ker.append([L.gamut_hip_gif_last_encode_kernel_ms(j) for j in range(5)])
        call = np.array(call[a.warmup:]); ker = np.array(ker[a.warmup:])
        med = np.median(ker, axis=0)
        mpx = n * a.frames * W * H / 1e6
        out_bytes = int(sum(olen))
        rows.append(json.dumps(dict(
            tool="gif_encode_bench", content=content, files=n, frames_per_file=a.frames, width=W, height=H, distinct_files=a.distinct,
            steps=a.steps, warmup=a.warmup, reference_repeats=a.ref_repeats, output_bytes=out_bytes, file_bytes=int(np.mean([len(r) for r in refs])),
            census_ms=round(float(med[0]), 3), plan_ms=round(float(med[1]), 3), lzw_ms=round(float(med[2]), 3), lzw_ms_min=round(float(ker[:, 2].min()), 3),
            offsets_ms=round(float(med[3]), 3), gather_ms=round(float(med[4]), 3),
            call_ms=round(float(np.median(call)), 3), call_ms_min=round(float(call.min()), 3),
            mpx_per_s=round(mpx / (float(np.median(call)) * 1e-3), 1),
            reference_one_core_ms_per_file=round(ref_ms, 2), reference_one_core_mpx_per_s=round(a.frames * W * H / 1e6 / (ref_ms * 1e-3), 1),
            reference_16_cores_ms_per_batch=round(ref_ms * n / 16, 1))))
        print(rows[-1], flush=True)
        del out
    if a.json:
        with open(a.json, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
