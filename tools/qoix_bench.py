"""QOIX decode throughput (gamut_hip_qoix_decode_batch_device), one JSON line per row, appended to profiles/qoix_bench.jsonl.

    python tools/qoix_bench.py [--images 1024] [--steps 5] [--warmup 2] [--cache DIR] [--json profiles/qoix_bench.jsonl]

Three 1920x1080 rgb8 files from the test generator (tests/qoix_gen.py), each repeated --images times: photo-like content stored, the
same op stream LZ4-compressed by the generator's greedy matcher (a few per cent smaller: real volume for the LZ4 kernel), and flat
content LZ4-compressed (a few hundred bytes of runs).  The generator is plain Python; --cache names a directory where the files are
kept between runs.  The library's decode
entry takes files in HOST memory; with GAMUT_HIP_QOIX_TIMING=1 (set here) it brackets its two kernels with events once the blob is
resident in HBM -- the "kernels" rows, split into the LZ4 and the op-stream kernel.  The whole call, staging and PCIe inside, is
reported separately ("file_level": true).  Medians of --steps calls after --warmup calls.  Every batch is checked against the C
restatement (tests/c/qoix_ref.c) on its first and last image before it is timed.  Yardsticks in the same process: the C restatement
on one host core (and that figure spread over 16 cores, by arithmetic: ms * images / 16), and gamut_hip_qoi_decode_batch_device on the
same pixels stored as QOI."""
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


def make_files(cache):
    """[(name, file bytes, pixels)]: photo-like stored, photo-like LZ4, flat LZ4"""
    import qoix_gen as G
    out = []
    for name, img, forms in (("photo-like", G.photo_like(W, H, 3, 101), ("stored", "LZ4")), ("flat", G.flat_image(W, H, 3, 102), ("LZ4",))):
        ops = None
        for form in forms:
            path = os.path.join(cache, f"qoix_bench_{name}_{form}_{W}x{H}.qoix") if cache else None
            if path and os.path.exists(path):
                f = open(path, "rb").read()
            else:
                ops = ops if ops is not None else G.encode_ops(img)
                f = G.stored(W, H, ops, 3) if form == "stored" else G.compressed(W, H, ops, 3)
                if path:
                    os.makedirs(cache, exist_ok=True)
                    open(path, "wb").write(f)
            out.append((f"{name}, {form}", f, img))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "qoix_bench.jsonl"))
    a = ap.parse_args()
    os.environ["GAMUT_HIP_QOIX_TIMING"] = "1"                          # read once by the library, at its first decode call
    import torch
    import qoix_ref_c
    from gamut_amd import _capi
    L = _capi.lib()
    _capi.check(L.gamut_hip_init(0))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    rows = []

    def emit(**kw):
        rows.append(json.dumps(dict(tool="qoix_bench", width=W, height=H, **kw)))
        print(rows[-1], flush=True)

    m = a.images
    ob = W * H * 3
    for name, f, img in make_files(a.cache):
        t = []
        for _ in range(3):
            t0 = time.perf_counter(); ref = qoix_ref_c.load(f, 0); t.append(1e3 * (time.perf_counter() - t0))
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
            run(); k0.append(L.gamut_hip_qoix_last_decode_stage_ms(0)); k1.append(L.gamut_hip_qoix_last_decode_stage_ms(1))
        k0, k1 = k0[a.warmup:], k1[a.warmup:]
        lz_ms, avg_ms = float(np.median(k0)), float(np.median(k1))
        nops = len(f) - 29 if not compression else int.from_bytes(f[25:29], "big") - 4
        if compression:
            emit(batch=f"decode {name}: k_qoix_lz4 (blob resident)", images=m, ms_per_batch=round(lz_ms, 3), ms_min=round(min(k0), 3), file_level=False,
                 bytes_in=m * len(f), bytes_out=m * (nops + 4), gb_per_s_out=round(m * (nops + 4) / (lz_ms * 1e-3) / 1e9, 2))
        emit(batch=f"decode {name}: k_qoix_avg (blob resident)", images=m, ms_per_batch=round(avg_ms, 3), ms_min=round(min(k1), 3), mpx_per_s=round(m * W * H / avg_ms / 1e3, 1),
             file_level=False, bytes_in=m * (nops + 29), bytes_out=m * ob, op_bytes_per_image=nops, ns_per_op_byte_per_wave=round(avg_ms * 1e6 / nops, 2),
             slower_than_restatement_on_16_cores=bool(avg_ms > host_ms * m / 16))
        ms, mn = timed(run, a.steps, a.warmup, torch.cuda.synchronize)
        emit(batch=f"decode {name}: whole call", images=m, ms_per_batch=round(ms, 3), ms_min=round(mn, 3), mpx_per_s=round(m * W * H / ms / 1e3, 1), file_level=True,
             bytes_in=m * len(f), bytes_out=m * ob, gb_per_s_files=round(m * len(f) / (ms * 1e-3) / 1e9, 2))
        if name.endswith("LZ4") and name.startswith("photo"):               # (the same pixels as the batch before: one yardstick per image)
            del out
            continue
        # ---- yardstick: the same pixels stored as QOI, through gamut_hip_qoi_decode_batch_device
        desc = _capi.QoiDesc(); desc.width, desc.height, desc.channels, desc.colorspace = W, H, 3, 0
        n = C.c_int(0)
        p = L.gamut_hip_qoi_encode(np.ascontiguousarray(img).ctypes.data, C.byref(desc), W * 3, C.byref(n))
        assert p, L.gamut_hip_last_error()
        qoi = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (n.value,)).copy()
        C.CDLL(None).free(C.c_void_p(p))
        qptrs = (C.c_void_p * m)(*([qoi.ctypes.data] * m)); qlens = (C.c_int * m)(*([qoi.size] * m))
        qdescs = (_capi.QoiDesc * m)()
        qrun = lambda: _capi.check(L.gamut_hip_qoi_decode_batch_device(qptrs, qlens, m, 0, offs, out.data_ptr(), qdescs, st, stream))
        qrun()
        assert np.array_equal(out[(m - 1) * ob:].cpu().numpy(), img.reshape(-1)), "QOI yardstick parity"
        ms, mn = timed(qrun, a.steps, a.warmup, torch.cuda.synchronize)
        emit(batch=f"yardstick gamut_hip_qoi_decode_batch_device, same pixels as QOI: {name.split(', ')[0]}", images=m, ms_per_batch=round(ms, 3), ms_min=round(mn, 3),
             mpx_per_s=round(m * W * H / ms / 1e3, 1), file_level=True, bytes_in=m * int(qoi.size), bytes_out=m * ob)
        del out
    if a.json:
        with open(a.json, "a") as fh:
            fh.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
