"""DDS / BC7 encode throughput (gamut_hip_dds_encode_batch_device), one JSON line per batch, appended to profiles/dds_encode_bench.jsonl.

    python tools/dds_encode_bench.py [--images 1024] [--steps 5] [--warmup 2] [--json profiles/dds_encode_bench.jsonl]

1920x1080 frames resident in HBM -> files in HBM: rgb8 and rgba8, photo-like and flat (tiles of one colour); the rgba8 photo carries
an alpha ramp over its left half, so those tiles take the encoder's alpha path.  With GAMUT_HIP_DDS_TIMING=1 (set here) the call
brackets its one launch with events: the "kernel" figure.  The whole call (upload of the image records and the wait inside) is
reported beside it.  The encoder is compute-bound, so the figures are megapixels per second; the bytes moved (pixels in, a quarter
as many bytes or fewer out) are far below what HBM carries in that time and no roofline fraction is given.  The yardstick is
k_convert_vec rgb8 -> rgba8 (gamut_hip_scanlines_convert_device) on the same frame count in the same process; the host figure is the
C restatement of the reference (tests/c/bc7_ref.c) on one core, the median of 3 encodes of one frame, and that figure divided by 16
for sixteen cores.  Every batch is checked byte for byte against that restatement on its first and last image before it is timed."""
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "dds_encode_bench.jsonl"))
    a = ap.parse_args()
    os.environ["GAMUT_HIP_DDS_TIMING"] = "1"                           # read once by the library, at its first encode call
    import torch
    import oracle_lib as O
    import bc7_ref_c
    from gamut_amd import _capi, synth
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(**kw):
        rows.append(json.dumps(dict(tool="dds_encode_bench", width=W, height=H, **kw)))
        print(rows[-1], flush=True)

    n = a.images
    photo = np.ascontiguousarray(synth.photo_rgb(W, H, 101))
    alpha = np.full((H, W), 255, np.uint8)
    alpha[:, :W // 2] = np.linspace(0, 255, W // 2).astype(np.uint8)[None, :]
    photo_a = np.ascontiguousarray(np.dstack([photo, alpha]))
    tiles = np.random.default_rng(7).integers(0, 256, (H // 120, W // 240, 4), dtype=np.uint8)
    flat_a = np.ascontiguousarray(np.repeat(np.repeat(tiles, 120, axis=0), 240, axis=1))
    flat = np.ascontiguousarray(flat_a[:, :, :3])
    # ---- yardstick: k_convert_vec rgb8 -> rgba8 on n frames
    src = torch.from_numpy(photo.reshape(-1)).to(dev).repeat(n)
    dst = torch.empty(n * W * H * 4, dtype=torch.uint8, device=dev)
    ms, mn = timed(lambda: _capi.check(L.gamut_hip_scanlines_convert_device(O.PT["rgb8"], src.data_ptr(), W * 3, W * H * 3, O.PT["rgba8"], dst.data_ptr(), W * 4, W * H * 4,
                                                                            W, H, n, stream)), a.steps, a.warmup, torch.cuda.synchronize)
    emit(batch="yardstick k_convert_vec rgb8->rgba8", images=n, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(n * W * H / ms / 1e3, 1))
    yard_mpx = n * W * H / ms / 1e3
    del dst, src
    for name, px in (("rgb8 photo-like", photo), ("rgba8 photo-like, alpha ramp on the left half", photo_a), ("rgb8 flat", flat), ("rgba8 flat", flat_a)):
        comp = px.shape[2]
        fb = W * H * comp
        want = bc7_ref_c.write_dds(px)
        t = []
        for _ in range(3):                                              # the C restatement on one host core
            t0 = time.perf_counter(); bc7_ref_c.write_dds(px); t.append(time.perf_counter() - t0)
        host_ms = 1e3 * float(np.median(t))
        s = torch.from_numpy(px.reshape(-1)).to(dev).repeat(n)
        bound = L.gamut_hip_dds_encode_bound(W, H, comp)
        assert bound == len(want)
        slot = (bound + 255) // 256 * 256
        out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
        ptrs = (C.c_void_p * n)(*[s.data_ptr() + i * fb for i in range(n)]); pitch = (C.c_int64 * n)(*([W * comp] * n))
        wa = (C.c_int32 * n)(*([W] * n)); ha = (C.c_int32 * n)(*([H] * n)); ca = (C.c_int32 * n)(*([comp] * n))
        offs = (C.c_int64 * n)(*[i * slot for i in range(n)]); lens = (C.c_int64 * n)(); st = (C.c_int * n)()
        run = lambda: _capi.check(L.gamut_hip_dds_encode_batch_device(ptrs, pitch, wa, ha, ca, n, offs, out.data_ptr(), lens, st, stream))
        run()
        assert list(lens) == [len(want)] * n, "encode length"
        for i in (0, n - 1):
            assert out[i * slot:i * slot + len(want)].cpu().numpy().tobytes() == want, "encode parity"
        kms = []
        for _ in range(a.warmup + a.steps):
            run()
            kms.append(L.gamut_hip_dds_last_encode_kernel_ms())
        kms = kms[a.warmup:]
        km = float(np.median(kms))
        ms, mn = timed(run, a.steps, a.warmup, torch.cuda.synchronize)
        blocks = np.frombuffer(want, np.uint8)[148:].reshape(-1, 16)
        emit(batch="encode " + name, images=n, kernel_ms=round(km, 3), kernel_ms_min=round(min(kms), 3), call_ms=round(ms, 3), call_ms_min=round(mn, 3),
             kernel_ms_per_frame=round(km / n, 4), mpx_per_s=round(n * W * H / km / 1e3, 1), bytes_out=n * len(want), file_bytes=len(want),
             mode1_fraction=round(float((blocks[:, 0] & 3 == 2).mean()), 4), yardstick_mpx_per_s_same_run=round(yard_mpx, 1),
             host_one_core_ms_per_frame=round(host_ms, 1), host_one_core_mpx_per_s=round(W * H / host_ms / 1e3, 2),
             host_16_cores_by_arithmetic_mpx_per_s=round(16 * W * H / host_ms / 1e3, 2))
        del out, s
    if a.json:
        with open(a.json, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
