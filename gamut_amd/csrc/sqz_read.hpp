// sqz_read.hpp -- the arithmetic of the device reader (sqz_read.hip), position by position: where the records of a sorting pass end,
// what each advances, which list entry it targets, and what the end of the stream does to the last one.  Plain functions for host and
// device: the kernels use them, and so does the serial stand-in for a workgroup that tools/sqz_read_fuzz_host.cpp runs under the
// sanitizers.  No function here reads a byte outside [file, file + len): bits outside the file read as 0.
//
// A SORTING PASS BY POSITION (SQZ_decode_sorting_pass, codecs/sqz.d:1988-2020, with SQZ_decode_read_wdr_run :1941-1951).  The pass
// starts at bit s.  A record is `sign, (0, b)*, 1`: even length, so every record starts at the parity of s, bits at ODD offsets from
// s are flags (a set flag closes a record) and bits at EVEN offsets are a record's sign (its first bit) or run data.  The run is
// (1 b1 .. bk) mod 2^32: the last 32 data bits -- the last 64 stream bits in front of the closing flag -- and k decide it.  The
// record advances ((run - 1) mod 2^32) + 1 entries of the LIP as it stood when the pass began.  THE END RULE: read_bit's -1 at the
// end of the stream is "not 0", so a stream that ends where a flag is due (N - s odd) closes the pending record there, with the run
// as read; a stream that ends at a sign or at a data position closes nothing.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SQZR_HD __host__ __device__ inline
#else
#define SQZR_HD inline
#endif

namespace gamut {

constexpr uint32_t kSqzrTaken = 0xFFFFFFFFu;                        // a LIP entry that left the list during the current pass (x | y << 16 never reaches it)

SQZR_HD uint32_t sqzr_byte(const uint8_t* file, uint64_t len, int64_t i) { return i >= 0 && (uint64_t)i < len ? file[i] : 0u; }

// the 32 bits at [pos, pos + 32), the first one on top; pos may be negative or behind the file
SQZR_HD uint32_t sqzr_bits32(const uint8_t* file, uint64_t len, int64_t pos)
{
    const int64_t b = pos >> 3;
    const uint32_t sh = (uint32_t)(pos & 7);
    uint64_t v = 0;
    for (int k = 0; k < 5; ++k) v = v << 8 | sqzr_byte(file, len, b + k);
    return (uint32_t)(v >> (8u - sh));
}
SQZR_HD uint64_t sqzr_bits64(const uint8_t* file, uint64_t len, int64_t pos)
{
    return (uint64_t)sqzr_bits32(file, len, pos) << 32 | sqzr_bits32(file, len, pos + 32);
}
SQZR_HD uint32_t sqzr_bit(const uint8_t* file, uint64_t len, int64_t pos) { return (sqzr_byte(file, len, pos >> 3) >> (7u - (uint32_t)(pos & 7))) & 1u; }

// SQZ_decode_init_subband's 4-bit read (:1896) at *pos < 8 * len: the value, or -1 with *pos at the end when the nibble straddles
// the file's last byte
SQZR_HD int sqzr_nibble(const uint8_t* file, uint64_t len, int64_t* pos)
{
    const int64_t p = *pos;
    if ((p & 7) > 4 && (uint64_t)(p >> 3) + 1u >= len) { *pos = (int64_t)(len * 8u); return -1; }
    *pos = p + 4;
    return (int)(sqzr_bits32(file, len, p) >> 28);
}

// The closing flags among the 32 bits `word` = [p, p + 32) of a pass that starts at s, p - s even, N = 8 * len: bit 31 - b set means
// a record closes at p + b.  The end rule puts one at N itself when N - s is odd; nothing lies behind N.
SQZR_HD uint32_t sqzr_flags(uint32_t word, int64_t p, int64_t s, int64_t N)
{
    const int64_t valid = N - p;
    if (valid <= 0) return 0u;
    uint32_t f = word & 0x55555555u;
    if (valid < 32) {
        f &= ~(0xFFFFFFFFu >> valid);
        if ((N - s) & 1) f |= 0x80000000u >> valid;
    }
    return f;
}

// the bits at even positions of q, packed: bit j of the result is bit 2j of q
SQZR_HD uint32_t sqzr_even_bits(uint64_t q)
{
    q &= 0x5555555555555555ull;
    q = (q | q >> 1) & 0x3333333333333333ull; q = (q | q >> 2) & 0x0F0F0F0F0F0F0F0Full; q = (q | q >> 4) & 0x00FF00FF00FF00FFull;
    q = (q | q >> 8) & 0x0000FFFF0000FFFFull; q = (q | q >> 16) & 0x00000000FFFFFFFFull;
    return (uint32_t)q;
}

// The record that closes at bit `flag` (a real flag or the end rule's) when the one before it closed at `prev` (s - 1 for the first
// of the pass): k = (flag - prev - 2) / 2 data bits at flag - 1, flag - 3, ..; the work does not depend on k or on the run.
SQZR_HD uint32_t sqzr_run(const uint8_t* file, uint64_t len, int64_t flag, int64_t prev)
{
    const uint64_t k = (uint64_t)(flag - prev - 2) >> 1;
    const uint32_t d = sqzr_even_bits(sqzr_bits64(file, len, flag - 64));
    return k >= 32u ? d : (1u << k) | (d & ((1u << k) - 1u));
}
SQZR_HD uint64_t sqzr_advance(uint32_t run) { return (uint64_t)(uint32_t)(run - 1u) + 1u; }      // run 0 advances 2^32
SQZR_HD uint32_t sqzr_sign(const uint8_t* file, uint64_t len, int64_t prev) { return sqzr_bit(file, len, prev + 1); }

// the refinement pass at pos with `lsp` merged entries: the bits it reads
SQZR_HD uint64_t sqzr_refine_bits(uint64_t lsp, int64_t pos, int64_t N) { const uint64_t left = pos < N ? (uint64_t)(N - pos) : 0u; return lsp < left ? lsp : left; }

// SQZ_decode_round_coefficients' mask (:2082-2103) for a band, 0 when the band is not rounded
SQZR_HD uint32_t sqzr_round_mask(int max_bitplane, int bitplane) { return max_bitplane == 0 || bitplane < 2 ? 0u : (((1u << bitplane) - 1u) ^ 1u) & 0xFFFFu; }

} // namespace gamut
