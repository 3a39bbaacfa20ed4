"""The host side of the PNG decoder without a GPU: tests/c/png_host_check.cpp, linked against gamut_amd/csrc/png_file.hip alone, on the corpus of
tests/png_host_corpus.py -- the slice plans of the device inflate (plan_slices), the gather of a stream's bytes from the IDAT chunks
(copy_idat_range), and the chunk walk with the IDAT bytes copied against the walk that only locates them, on whole, re-chunked and truncated files."""
import os
import re
import subprocess

import png_host_corpus

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_corpus_has_what_the_check_is_about():
    files = png_host_corpus.corpus()
    assert [f for f, _ in files[:5]] == [open(os.path.join(HERE, "golden", "ref_images", n), "rb").read() for n in png_host_corpus.FIXTURES]
    gen_files = png_host_corpus.generated()
    assert len(gen_files) >= 2 * 15 and all(len(f) < 1000 for f in gen_files)           # (a 256-entry PLTE is 768 bytes)
    for f in gen_files:
        r = png_host_corpus.rechunk(f)
        idats = [d for t, d in png_host_corpus.chunks(r) if t == b"IDAT"]
        assert len(idats) >= 2 and all(len(d) == 1 for d in idats)                       # the zlib header spans two chunks
        assert b"".join(idats) == b"".join(d for t, d in png_host_corpus.chunks(f) if t == b"IDAT")
        assert [c for c in png_host_corpus.chunks(r) if c[0] != b"IDAT"] == [c for c in png_host_corpus.chunks(f) if c[0] != b"IDAT"]


def test_png_host_check(tmp_path):
    """builds the check with hipcc (host code only, no sanitizer) and runs it; it exits non-zero at the first assertion that does not hold"""
    exe, corpus = str(tmp_path / "png_host_check"), str(tmp_path / "corpus.bin")
    files = png_host_corpus.write(corpus)
    csrc = os.path.join(ROOT, "gamut_amd", "csrc")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-I", csrc, os.path.join(HERE, "c", "png_host_check.cpp"),
                           os.path.join(csrc, "png_file.hip"), "-o", exe, "-lz"])
    out = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.search(r"(\d+) slice plans, (\d+) gathered ranges, (\d+) files \((\d+) whole, the rest truncations\): (\d+) accepted, zlib header ok (\d+) / bad (\d+)", out.stdout)
    assert m, out.stdout
    plans, ranges, n_files, whole, accepted, zlib_ok, zlib_bad = map(int, m.groups())
    assert plans >= 2 * 2 * 3 * 11 + 2 and ranges == 2 * (1000 + 994 + 937 + 998 + 992 + 935)
    assert whole == len(files) and n_files == whole + sum(len(f) for f, t in files if t)
    assert accepted > whole // 2 and zlib_ok > 100 and zlib_bad > 0
