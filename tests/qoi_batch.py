"""Launch layouts for the QOI decode kernels (gamut_amd/csrc/qoi.hip), built on the host with no GPU in them: which streams of tests/qoi_cases.py
go into one call, where each lies in the blob (or in host memory), where its pixels go, and what the WHOLE output allocation must hold afterwards.
tests/test_qoi_batch_gpu.py hands the tables to the library and compares the allocation; tests/test_qoi_cases_cpu.py checks the layouts themselves.

Every array a C call reads is an attribute of the layout and lives as long as the layout does.  A pointer is taken with pointer(layout, "name"),
from the attribute, never from an expression: `np.array(...).ctypes.data` is the address of a temporary that numpy frees before the call (or the
asynchronous copy behind it) reads it."""
import collections
import ctypes as C

import numpy as np

import qoi_cases as Q

SLACK = 160                                          # GAMUT_HIP_QOI_SLACK (include/gamut_hip.h; test_qoi_cases_cpu.py compares the two)
POISON = 0x5A
FILLS = ("zeros", "0xFF", "0xFE", "0xFD", "noise", "stream")        # what lies between the streams; 0xFD is a RUN of 62, 0xFE / 0xFF start RGB / RGBA ops
DESC = np.dtype([("width", "<u4"), ("height", "<u4"), ("channels", "u1"), ("colorspace", "u1")], align=True)      # gamut_hip_qoi_desc

Stream = collections.namedtuple("Stream", "case copy fill")
Difference = collections.namedtuple("Difference", "case copy byte pixel text")


def pointer(layout, name, ctype):
    """a pointer to the array layout.<name>: the attribute itself, which lives as long as the layout"""
    arr = getattr(layout, name)
    assert isinstance(arr, np.ndarray) and arr.flags.c_contiguous and arr.flags.owndata
    return arr.ctypes.data_as(C.POINTER(ctype))


class _Layout:
    """the streams of one call, in order, and their places in the output allocation"""

    def __init__(self, cases, channels, copies, seed, count=None, expected=Q.expected):
        """expected(name, channels): the oracle's pixels of a case, flat (the default knows the cases of tests/qoi_cases.py)"""
        assert channels in (0, 3, 4) and copies >= 1
        self.channels, self.copies, self.seed, self.expected = channels, copies, seed, expected
        rng = np.random.default_rng(seed)
        every = [Stream(c, k, FILLS[(k + j) % len(FILLS)]) for k in range(copies) for j, c in enumerate(cases)]
        self.streams = [every[i] for i in rng.permutation(len(every))][:count]          # a seeded permutation: long streams beside short ones
        self.n = len(self.streams)
        self.out_channels = np.array([channels or Q.header(s.case.data)[2] for s in self.streams], np.int32)
        self.out_bytes = np.array([expected(s.case.name, channels).size for s in self.streams], np.int64)
        # a gap of 1 to 67 bytes in front of every image and behind the last; the three- and the four-channel images each start at every residue mod 16 in turn
        self.out_offset = np.zeros(self.n, np.int64)
        pos, turn = 0, {3: 0, 4: 0}
        for i in range(self.n):
            ch = int(self.out_channels[i])
            want = (7 * turn[ch] + 3) % 16; turn[ch] += 1
            gap = int(rng.integers(1, 52))
            gap += (want - (pos + gap)) % 16
            assert 1 <= gap <= 67
            self.out_offset[i] = pos + gap
            pos += gap + int(self.out_bytes[i])
        self.out_len = pos + int(rng.integers(1, 68))
        self.poison = np.full(self.out_len, POISON, np.uint8)
        self._rng, self._expected = rng, None

    def expected_allocation(self):
        """the whole output buffer as it must look afterwards: POISON everywhere, the oracle's pixels at each offset"""
        if self._expected is None:                                                        # computed once, shared, read-only
            exp = np.full(self.out_len, POISON, np.uint8)
            for s, off, nb in zip(self.streams, self.out_offset, self.out_bytes):
                exp[off:off + nb] = self.expected(s.case.name, self.channels)
            exp.setflags(write=False)
            self._expected = exp
        return self._expected

    def first_difference(self, got):
        """None, or where the first wrong byte lies: the case and copy, the byte offset within its image and the pixel number (negative in front
        of the first image; at or past the image's size: the gap behind it)"""
        exp = self.expected_allocation()
        if got.shape != exp.shape:
            return Difference(None, None, None, None, f"{got.size} bytes, not {exp.size}")
        bad = np.flatnonzero(got != exp)
        if bad.size == 0:
            return None
        at = int(bad[0])
        i = max(int(np.searchsorted(self.out_offset, at, side="right")) - 1, 0)
        s, byte, ch = self.streams[i], at - int(self.out_offset[i]), int(self.out_channels[i])
        inside = 0 <= byte < int(self.out_bytes[i])
        where = f"byte {byte} (pixel {byte // ch}, channel {byte % ch}) of {int(self.out_bytes[i])}" if inside else f"the gap {'behind' if byte > 0 else 'in front of'} it (byte {byte})"
        names = self.wrong_cases(got)
        text = (f"{s.case.name}, copy {s.copy} (stream {i} of {self.n}, {ch} channels out, fill {s.fill}): {where} is {int(got[at]):#04x}, not {int(exp[at]):#04x}; "
                f"{bad.size} bytes differ in the allocation, in the images of {len(names)} cases: {' '.join(names)}")
        return Difference(s.case.name, s.copy, byte, byte // ch, text)

    def wrong_cases(self, got):
        """the names of the cases with a wrong byte inside an image of theirs, sorted"""
        exp = self.expected_allocation()
        return sorted({s.case.name for s, off, nb in zip(self.streams, self.out_offset, self.out_bytes) if not np.array_equal(got[off:off + nb], exp[off:off + nb])})


class ResidentLayout(_Layout):
    """everything one gamut_hip_qoi_decode_resident_device call needs: blob (blob_len bytes), begin, size, descs, out_offset, poison"""

    def __init__(self, cases, channels, copies, seed, count=None, expected=Q.expected):
        super().__init__(cases, channels, copies, seed, count, expected)
        rng = self._rng
        self.size = np.array([len(s.case.data) for s in self.streams], np.int32)
        # an odd base offset; stream i begins at residue 37 i + 1 mod 64 (37 is odd: neighbours differ and every residue comes up); at least
        # SLACK bytes behind each stream, and exactly SLACK behind the last
        self.begin = np.zeros(self.n, np.int64)
        pos = 0
        for i in range(self.n):
            pos += ((37 * i + 1) - pos) % 64
            self.begin[i] = pos
            pos += int(self.size[i]) + SLACK
        self.blob_len = pos
        self.blob = np.zeros(self.blob_len, np.uint8)
        edges = [0] + [int(b + z) for b, z in zip(self.begin, self.size)]                  # gap k: in front of stream k (its own fill), the last: behind the last stream
        for k in range(self.n + 1):
            s = self.streams[min(k, self.n - 1)]
            lo, hi = edges[k], int(self.begin[k]) if k < self.n else self.blob_len
            self.blob[lo:hi] = self._fill(s, hi - lo, rng)
        for s, b, z in zip(self.streams, self.begin, self.size):
            self.blob[b:b + z] = np.frombuffer(s.case.data, np.uint8)
        self.descs = np.zeros(self.n, DESC)
        for i, s in enumerate(self.streams):
            self.descs[i] = Q.header(s.case.data) + (s.case.data[13],)
        self.descs_read = np.zeros(self.n, DESC)                                          # what the library's header reader says (fill_descs)

    @staticmethod
    def _fill(s, n, rng):
        if s.fill == "noise":
            return rng.integers(0, 256, n, dtype=np.uint8)
        if s.fill == "stream":                                                            # the first bytes of the stream itself, header and all, over and over
            return np.resize(np.frombuffer(s.case.data, np.uint8), n) if n else np.zeros(0, np.uint8)
        return np.full(n, {"zeros": 0, "0xFF": 0xFF, "0xFE": 0xFE, "0xFD": 0xFD}[s.fill], np.uint8)

    def fill_descs(self, read_header, desc_type):
        """descs_read through the library's header reader (gamut_hip_qoi_read_header), stream by stream, from the bytes in the blob"""
        base = pointer(self, "descs_read", desc_type)
        for i in range(self.n):
            rc = read_header(self.blob.ctypes.data + int(self.begin[i]), int(self.size[i]), C.byref(base[i]))
            assert rc == 0, self.streams[i].case.name
        assert self.descs_read.tobytes() == self.descs.tobytes()

    def tables(self):
        """name -> (pointer, bytes behind it) of every host table the call reads"""
        return {"begin": (pointer(self, "begin", C.c_int64), self.begin.nbytes), "size": (pointer(self, "size", C.c_int), self.size.nbytes),
                "descs": (pointer(self, "descs", C.c_uint8), self.descs.nbytes), "descs_read": (pointer(self, "descs_read", C.c_uint8), self.descs_read.nbytes),
                "out_offset": (pointer(self, "out_offset", C.c_int64), self.out_offset.nbytes), "blob": (pointer(self, "blob", C.c_uint8), self.blob.nbytes),
                "poison": (pointer(self, "poison", C.c_uint8), self.poison.nbytes)}


class HostLayout(_Layout):
    """everything one gamut_hip_qoi_decode_batch_device call needs: the files in host memory (files[i], each an array of its own), ptrs, size,
    out_offset, poison; descs_read and status are what the call fills"""

    def __init__(self, cases, channels, copies, seed, count=None, expected=Q.expected):
        super().__init__(cases, channels, copies, seed, count, expected)
        self.files = [np.frombuffer(s.case.data, np.uint8).copy() for s in self.streams]
        self.ptrs = np.array([f.ctypes.data for f in self.files], np.uintp)
        self.size = np.array([f.size for f in self.files], np.int32)
        self.descs_read = np.zeros(self.n, DESC)
        self.status = np.full(self.n, -1, np.int32)

    def tables(self):
        return {"ptrs": (pointer(self, "ptrs", C.c_void_p), self.ptrs.nbytes), "size": (pointer(self, "size", C.c_int), self.size.nbytes),
                "out_offset": (pointer(self, "out_offset", C.c_int64), self.out_offset.nbytes), "descs_read": (pointer(self, "descs_read", C.c_uint8), self.descs_read.nbytes),
                "status": (pointer(self, "status", C.c_int), self.status.nbytes), "poison": (pointer(self, "poison", C.c_uint8), self.poison.nbytes)}


ONE_WAVE_COPIES = 7                                  # 7 x 122 = 854 streams: at least Q.WIDE_BELOW, one launch of k_qoi_decode<1>


def resident(kernel, channels):
    """the layouts of test_every_case_resident: "one_wave" is seven copies of the case list, the small-batch kernels get one"""
    return ResidentLayout(Q.CASES, channels, ONE_WAVE_COPIES if kernel == "one_wave" else 1, 1000 + channels)


def threshold(count, channels):
    """the first `count` streams of the seven-copy list (test_both_sides_of_the_wide_threshold)"""
    return ResidentLayout(Q.CASES, channels, ONE_WAVE_COPIES, 1000 + channels, count)


def host(copies, channels):
    """every case, `copies` times, from host memory (test_constructed_cases_from_host_memory): one launch up to Q.HOST_GROUP streams"""
    return HostLayout(Q.CASES, channels, copies, 2000 + 10 * copies + channels)


def alone(case, channels=4):
    """one case as a batch of one"""
    return HostLayout([case], channels, 1, 3000)


DROP_IN_FAMILIES = ("straddle-window", "straddle-lane", "straddle-end", "chunk", "buffer", "full", "index", "alpha")


def drop_in_cases():
    """one constructed case of each family, for gamut_hip_qoi_decode: the last of the family in the list"""
    return [[c for c in Q.CONSTRUCTED if c.name.startswith(f + "-")][-1] for f in DROP_IN_FAMILIES]
