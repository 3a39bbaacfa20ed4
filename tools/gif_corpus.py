"""Writes the corpus for tests/c/gif_host_check.cpp: every generated case of tests/gif_cases.py, the fixture, the larger files, 25 000
mutated small files and truncations of the first 90 files at every seventh length, each as a little-endian u32 length and the bytes.

    python tools/gif_corpus.py corpus.bin"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import gif_cases
    fixture = open(os.path.join(ROOT, "tests", "golden", "gif", "animated_loop.gif"), "rb").read()
    fs = [f for _, f, _ in gif_cases.cases()] + [gif_cases.three_frames(), gif_cases.large(), fixture, b"", b"GIF89a"]
    fs += gif_cases.mutated(20000, 5) + gif_cases.mutated(5000, 77)
    fs += [f[:k] for f in fs[:90] for k in range(0, min(len(f), 400), 7)]
    with open(sys.argv[1], "wb") as o:
        for f in fs:
            o.write(struct.pack("<I", len(f)) + f)
    print(len(fs), "files")


if __name__ == "__main__":
    main()
