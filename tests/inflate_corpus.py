"""What tests/test_inflate_gpu.py and tests/test_inflate_cases_*.py share: the encoder-made corpus (zlib at every setting), the call into
gamut_hip_inflate_batch_device[_sliced], and the list of the encoder-made streams the census of tests/test_inflate_cases_cpu.py walks."""
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (run as a script: the package lies next to tests/)
from gamut_amd import _capi  # noqa: E402


def _deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=-15, mem=8, flush_every=0):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    if not flush_every:
        return co.compress(data) + co.flush()
    out = []
    for i in range(0, len(data), flush_every):
        out.append(co.compress(data[i:i + flush_every]))
        out.append(co.flush(zlib.Z_FULL_FLUSH if (i // flush_every) % 2 else zlib.Z_SYNC_FLUSH))
    out.append(co.flush())
    return b"".join(out)


def zlib_inflate(data):
    """zlib on a raw DEFLATE stream -> the bytes, or None where zlib turns the stream away or wants more input"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(data)
    except zlib.error:
        return None
    return out if d.eof else None


def _inflate_device(L, streams, caps, slice_bytes=0):
    """streams: list of raw-deflate byte strings; caps: output capacities -> (rc, [bytes], [status])"""
    n = len(streams)
    offs = np.concatenate([[0], np.cumsum([len(s) + 3 for s in streams])]).astype(np.int64)      # odd offsets: no alignment promised
    blob = np.zeros(int(offs[-1]) + 1, np.uint8)
    for i, s in enumerate(streams):
        blob[offs[i]:offs[i] + len(s)] = np.frombuffer(s, np.uint8)
    ooffs = np.concatenate([[0], np.cumsum([c + 5 for c in caps])]).astype(np.int64)
    dblob = L.gamut_hip_device_malloc(blob.size + 64); dout = L.gamut_hip_device_malloc(int(ooffs[-1]) + 64)
    dlen = L.gamut_hip_device_malloc(4 * n + 16); dst = L.gamut_hip_device_malloc(4 * n + 16)
    poison = np.full(int(ooffs[-1]) + 64, 0xA5, np.uint8)
    _capi.check(L.gamut_hip_memcpy_h2d(dblob, blob.ctypes.data, blob.size, None))
    _capi.check(L.gamut_hip_memcpy_h2d(dout, poison.ctypes.data, poison.size, None))
    descs = (_capi.InflateDesc * n)()
    for i in range(n):
        descs[i].src = dblob + int(offs[i]); descs[i].dst = dout + int(ooffs[i]); descs[i].src_len = len(streams[i]); descs[i].dst_cap = caps[i]
    _capi.check(L.gamut_hip_stream_synchronize(None))
    rc = L.gamut_hip_inflate_batch_device_sliced(descs, n, dlen, dst, slice_bytes, None) if slice_bytes else L.gamut_hip_inflate_batch_device(descs, n, dlen, dst, None)
    lens = np.zeros(n, np.uint32); st = np.zeros(n, np.uint32); host = np.empty(poison.size, np.uint8)
    _capi.check(L.gamut_hip_memcpy_d2h(lens.ctypes.data, dlen, 4 * n, None))
    _capi.check(L.gamut_hip_memcpy_d2h(st.ctypes.data, dst, 4 * n, None))
    _capi.check(L.gamut_hip_memcpy_d2h(host.ctypes.data, dout, host.size, None))
    _capi.check(L.gamut_hip_stream_synchronize(None))
    for p in (dblob, dout, dlen, dst):
        L.gamut_hip_device_free(p)
    outs = []
    for i in range(n):
        outs.append(host[ooffs[i]:ooffs[i] + lens[i]].tobytes())
        assert (host[ooffs[i] + caps[i]:ooffs[i + 1]] == 0xA5).all(), f"stream {i} wrote past its capacity"
    return rc, outs, list(st)


def _corpus():
    rng = np.random.default_rng(11)
    noise = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    text = (b"the quick brown fox jumps over the lazy dog. " * 3000)[:120000]
    grad = (np.add.outer(np.arange(300), np.arange(400)) // 3 % 256).astype(np.uint8).tobytes()
    lownoise = (rng.integers(0, 4, 200000, dtype=np.uint8) + (np.arange(200000) // 997 % 200).astype(np.uint8)).tobytes()
    sparse = np.where(rng.random(150000) < 0.02, rng.integers(1, 256, 150000), 0).astype(np.uint8).tobytes()
    far = noise[:32768] + noise[:32768] + noise[100:30000] + bytes(70000) + noise[:5000]         # distances up to the whole window
    return {"noise": noise, "text": text, "grad": grad, "lownoise": lownoise, "sparse": sparse, "far": far, "empty": b"", "one": b"x",
            "runs": b"a" * 100000 + b"ab" * 40000 + b"abc" * 30000}


def corpus_settings():
    """the eleven encoder settings test_inflate_matches_zlib_on_every_encoder_setting runs every corpus entry under: (name, _deflate keywords)"""
    out = [(f"level {level}", dict(level=level)) for level in (0, 1, 6, 9)]
    out += [(sn, dict(level=6, strategy=strat)) for strat, sn in ((zlib.Z_FIXED, "fixed"), (zlib.Z_HUFFMAN_ONLY, "huffman-only"), (zlib.Z_RLE, "rle"), (zlib.Z_FILTERED, "filtered"))]
    out += [("flushed every 777", dict(level=6, flush_every=777)), ("memLevel 1 (small blocks)", dict(level=9, mem=1)), ("512-byte window", dict(level=6, wbits=-9))]
    return out


def corpus_streams():
    """(name, stream) of every corpus entry under every setting: the streams of the first test of tests/test_inflate_gpu.py, in its order"""
    for name, data in _corpus().items():
        for sn, kw in corpus_settings():
            yield f"{name} {sn}", _deflate(data, **kw)


def large_streams():
    """(name, stream) of the multi-megabyte streams of tests/test_inflate_gpu.py (capacity, round-and-tile, sliced and scratch tests; one
    stream per distinct input and setting, the repeats at other capacities left out), written out again here from the tests' own generators as they
    stood when the census was taken: no test runs this, so it is a snapshot, not a view of what those tests feed today.  Minutes in the pure-Python
    reference: walked once by `python tests/inflate_corpus.py` -- DESIGN.md 4.7.1 holds the result."""
    rng = np.random.default_rng(5)
    big = (rng.integers(0, 16, 6_000_000, dtype=np.uint8) * 3 + (np.arange(6_000_000) // 4093 % 100).astype(np.uint8)).tobytes()
    yield "capacity: big level 6", _deflate(big, 6)
    yield "rejects: text[:30000] level 6", _deflate(_corpus()["text"][:30000], 6)
    rng = np.random.default_rng(3)
    data = (rng.integers(0, 8, 30000, dtype=np.uint8) * 9).tobytes()
    yield "blocks: flushed every 23", _deflate(data, 6, flush_every=23)
    yield "blocks: fixed, flushed every 400", _deflate(data, 6, zlib.Z_FIXED, flush_every=400)
    rng = np.random.default_rng(23)
    seed = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    two = rng.integers(0, 2, 3_000_000, dtype=np.uint8).tobytes()
    cases = {
        "zeros": bytes(5_000_000),
        "period 3": b"\x10\x80\xf0" * 1_200_000,
        "period 259": rng.integers(0, 256, 259, dtype=np.uint8).tobytes() * 12000,
        "period 32768": seed * 40,
        "period 32768 with edits": b"".join(seed[:k * 811 % 32768] + b"!" + seed[k * 811 % 32768 + 1:] for k in range(30)),
        "two symbols": two,
        "runs between noise": b"".join(rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() + bytes([int(n) & 255]) * int(40000 + n) for n in rng.integers(1, 3000, 25)),
    }
    for name, data in cases.items():
        for kw in (dict(level=6), dict(level=9), dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY), dict(level=6, strategy=zlib.Z_RLE), dict(level=1, mem=1)):
            if name == "two symbols" and kw.get("strategy") != zlib.Z_HUFFMAN_ONLY and kw.get("level") != 1:
                continue
            yield f"tiles: {name} {kw}", _deflate(data, **kw)
    rng = np.random.default_rng(31)
    corpus = _corpus()
    big = (rng.integers(0, 16, 3_000_000, dtype=np.uint8) * 3 + (np.arange(3_000_000) // 4093 % 100).astype(np.uint8)).tobytes()
    noise = rng.integers(0, 256, 1_500_000, dtype=np.uint8).tobytes()
    for dn, data in (("big", big), ("noise", noise), ("runs x 6", corpus["runs"] * 6), ("far x 5", corpus["far"] * 5), ("zeros", bytes(2_000_000))):
        for kw in (dict(level=6), dict(level=1, mem=1), dict(level=0), dict(level=6, strategy=zlib.Z_FIXED), dict(level=6, flush_every=50000)):
            yield f"sliced: {dn} {kw}", _deflate(data, **kw)
    rng = np.random.default_rng(23)
    for i in range(150):
        yield f"scratch: {i}", _deflate(rng.integers(0, 64, 3000 + 17 * i, dtype=np.uint8).tobytes(), 6)


def census_of(streams):
    """the merged census (tests/inflate_ref.py) of (name, stream) pairs, and the name of the stream that set each maximum"""
    import inflate_ref as R
    total, holder = R.Census(), {}
    for name, s in streams:
        _, cs = R.inflate(s, memo=True)
        for k in ("max_lit_len", "max_dist_len", "max_cl_bits", "max_round_tokens", "max_same_dist_run", "max_long_per_tile"):
            if getattr(cs, k) > getattr(total, k):
                holder[k] = name
        cs.blocks = []                                         # (the per-block records of megabytes of small blocks are not kept)
        total.merge(cs)
    return total, holder


def census_row(cs):
    return {"max literal / length code used": cs.max_lit_len, "max distance code used": cs.max_dist_len, "longest code-length stream (bits)": cs.max_cl_bits,
            "hlit": (min(cs.hlit), max(cs.hlit)) if cs.hlit else None, "hdist": (min(cs.hdist), max(cs.hdist)) if cs.hdist else None,
            "hclen": (min(cs.hclen), max(cs.hclen)) if cs.hclen else None, "distance codes per block, fewest": min(cs.dist_code_sizes) if cs.dist_code_sizes else None,
            "distance symbols used": len(cs.dist_syms), "length symbols used": len(cs.len_syms), "258 as 284 + 31": cs.spelled_258_as_284,
            "most tokens within 32 KiB of input": cs.max_round_tokens, "longest same-distance run": cs.max_same_dist_run,
            "most long matches per 28 KiB of output": cs.max_long_per_tile, "tokens": cs.tokens, "rounds": cs.rounds}


if __name__ == "__main__":                                     # the census of the whole existing suite, one process per stream
    import multiprocessing

    def one(item):
        return item[0], census_of([item])[0]

    for title, gen_ in (("corpus x settings", corpus_streams), ("large streams", large_streams)):
        total = None
        with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
            for name, cs in pool.imap_unordered(one, list(gen_())):
                total = cs if total is None else total.merge(cs)
        print(title)
        for k, v in census_row(total).items():
            print(f"  {k}: {v}")
