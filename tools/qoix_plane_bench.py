"""QOI-Plane decode throughput (QOIX grey files through gamut_hip_qoix_decode_batch_device with gamut_hip_qoix_set_plane(1)), one JSON
line per row, appended to profiles/qoix_plane_bench.jsonl.

    python tools/qoix_plane_bench.py [--images 1024] [--steps 5] [--warmup 2] [--cache DIR] [--json profiles/qoix_plane_bench.jsonl]

Four 1920x1080 files from the test generator (tests/qoiplane_gen.py), each repeated --images times: photo-like l8 stored, the same op
stream LZ4-compressed, photo-like la8 stored, flat l8 stored.  The generator is plain Python; --cache names a directory where the files
are kept between runs.  With GAMUT_HIP_QOIX_TIMING=1 (set here) the decode call brackets its kernels with events once the blob is
resident in HBM -- the "kernels" rows, k_qoix_lz4 and k_qoix_plane.  The whole call, staging and PCIe inside, is reported separately
("file_level": true).  Medians of --steps calls after --warmup calls.  Every batch is checked against the C restatement
(tests/c/qoiplane_ref.c) on its first and last image before it is timed.  Yardsticks in the same process: the C restatement on one host
core (and that figure spread over 16 cores, by arithmetic: ms * images / 16), and k_qoix_avg on an rgb8 version of the photo-like
picture (the luminance in all three channels, encoded by tests/qoix_gen.py)."""
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


def cached(cache, name, make):
    path = os.path.join(cache, f"qoix_plane_bench_{name}_{W}x{H}.qoix") if cache else None
    if path and os.path.exists(path):
        return open(path, "rb").read()
    f = make()
    if path:
        os.makedirs(cache, exist_ok=True)
        open(path, "wb").write(f)
    return f


def make_files(cache):
    """[(name, file bytes, pixels)] and the rgb8 yardstick file"""
    import qoiplane_gen as P
    import qoix_gen as G
    photo, photo_la, flat = P.photo_like(W, H, 1, 101), P.photo_like(W, H, 2, 101), P.flat_image(W, H, 1, 102)
    files = [("photo-like l8, stored", cached(cache, "photo_l8_stored", lambda: P.encode(photo)), photo),
             ("photo-like l8, LZ4", cached(cache, "photo_l8_lz4", lambda: P.encode(photo, lz4=True)), photo),
             ("photo-like la8, stored", cached(cache, "photo_la8_stored", lambda: P.encode(photo_la)), photo_la),
             ("flat l8, stored", cached(cache, "flat_l8_stored", lambda: P.encode(flat)), flat)]
    rgb = np.repeat(photo, 3, axis=2)
    return files, (cached(cache, "photo_rgb8_stored", lambda: G.encode(rgb)), rgb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "qoix_plane_bench.jsonl"))
    ap.add_argument("--files-only", action="store_true", help="write the files into --cache and stop (no GPU needed)")
    a = ap.parse_args()
    files, (rgb_file, rgb) = make_files(a.cache)
    if a.files_only:
        return
    os.environ["GAMUT_HIP_QOIX_TIMING"] = "1"                          # read once by the library, at its first decode call
    import torch
    import qoiplane_ref_c
    from gamut_amd import _capi
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    previous = L.gamut_hip_qoix_set_plane(1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(**kw):
        rows.append(json.dumps(dict(tool="qoix_plane_bench", width=W, height=H, **kw)))
        print(rows[-1], flush=True)

    m = a.images
    host_photo_ms = None
    for name, f, img in files + [("photo-like rgb8 (QOI2AVG yardstick), stored", rgb_file, rgb)]:
        ch = img.shape[2]
        ob = W * H * ch
        kernel = "k_qoix_plane" if ch < 3 else "k_qoix_avg"
        t = []
        for _ in range(3):
            t0 = time.perf_counter(); ref = qoiplane_ref_c.load(f, 0); t.append(1e3 * (time.perf_counter() - t0))
        host_ms = float(np.median(t))
        assert np.array_equal(ref[0], img), "the restatement does not give the generator's pixels back"
        compression = f[16]
        emit(batch=f"C restatement, one host core: {name}", images=1, ms_per_batch=round(host_ms, 3), mpx_per_s=round(W * H / host_ms / 1e3, 1), file_level=True,
             file_bytes=len(f), compression=compression)
        emit(batch=f"C restatement spread over 16 host cores (arithmetic): {name}", images=m, ms_per_batch=round(host_ms * m / 16, 3),
             mpx_per_s=round(16 * W * H / host_ms / 1e3, 1), file_level=True)
        buf = np.frombuffer(f, np.uint8)
        ptrs = (C.c_void_p * m)(*([buf.ctypes.data] * m)); lens = (C.c_size_t * m)(*([buf.size] * m))
        offs = (C.c_int64 * m)(*[i * ob for i in range(m)])
        out = torch.empty(m * ob, dtype=torch.uint8, device=dev)
        st = (C.c_int * m)()
        run = lambda: _capi.check(L.gamut_hip_qoix_decode_batch_device(ptrs, lens, m, 0, offs, out.data_ptr(), None, st, stream))
        run()
        assert np.array_equal(out[:ob].cpu().numpy(), ref[0].reshape(-1)) and np.array_equal(out[(m - 1) * ob:].cpu().numpy(), ref[0].reshape(-1)), "decode parity"
        k0, k1 = [], []
        for _ in range(a.warmup + a.steps):
            run(); k0.append(L.gamut_hip_qoix_last_decode_stage_ms(0)); k1.append(L.gamut_hip_qoix_last_plane_kernel_ms() if ch < 3 else L.gamut_hip_qoix_last_decode_stage_ms(1))
        k0, k1 = k0[a.warmup:], k1[a.warmup:]
        lz_ms, op_ms = float(np.median(k0)), float(np.median(k1))
        nops = len(f) - 29 if not compression else int.from_bytes(f[25:29], "big") - 4
        if compression:
            emit(batch=f"decode {name}: k_qoix_lz4 (blob resident)", images=m, ms_per_batch=round(lz_ms, 3), ms_min=round(min(k0), 3), file_level=False,
                 bytes_in=m * len(f), bytes_out=m * (nops + 4), gb_per_s_out=round(m * (nops + 4) / (lz_ms * 1e-3) / 1e9, 2))
        emit(batch=f"decode {name}: {kernel} (blob resident)", images=m, ms_per_batch=round(op_ms, 3), ms_min=round(min(k1), 3), mpx_per_s=round(m * W * H / op_ms / 1e3, 1),
             file_level=False, bytes_in=m * (nops + 29), bytes_out=m * ob, op_bytes_per_image=nops, ns_per_pixel_per_wave=round(op_ms * 1e6 / (W * H), 2),
             slower_than_restatement_on_16_cores=bool(op_ms > host_ms * m / 16))
        ms, mn = timed(run, a.steps, a.warmup, torch.cuda.synchronize)
        emit(batch=f"decode {name}: whole call", images=m, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(m * W * H / ms / 1e3, 1), file_level=True,
             bytes_in=m * len(f), bytes_out=m * ob, gb_per_s_files=round(m * len(f) / (ms * 1e-3) / 1e9, 2))
        del out
    L.gamut_hip_qoix_set_plane(previous)
    if a.json:
        with open(a.json, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
