// device_util.hpp -- device helpers the codec kernels share: units -> records, bounds-checked file reads, byte runs out of LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gamut {

// The record that owns unit u.  A batch's records (images, files) are in unit order and each holds the number of its first unit in
// the member `First` (&DecImg::unit0, &EncImg::tile0, &PImg::row0, ...): the last record whose first unit is <= u.
template <auto First, class Rec> __device__ __forceinline__ int find_unit(const Rec* recs, int n, uint32_t u)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (recs[mid].*First <= u) lo = mid; else hi = mid - 1; }
    return lo;
}

// A file of the batch's blob: rec.file is the device address of its byte 0, positions >= rec.avail read as zero and are never loaded.
// file_dword: pos is a multiple of 4 from an aligned position; a dword that begins inside the file ends inside the blob.
template <class Rec> __device__ __forceinline__ uint32_t file_dword(const Rec& rec, uint64_t pos)
{
    return pos < rec.avail ? *reinterpret_cast<const uint32_t*>(rec.file + pos) : 0u;
}
template <class Rec> __device__ __forceinline__ uint32_t file_byte(const Rec& rec, uint64_t pos) { return pos < rec.avail ? rec.file[pos] : 0u; }

// byte k of a little-endian dword array
__device__ __forceinline__ uint32_t byte_of(const uint32_t* v, uint32_t k) { return (v[k >> 2] >> (8 * (k & 3))) & 255u; }
__device__ __forceinline__ void set_byte(uint32_t* v, int k, uint32_t b) { v[k >> 2] |= b << (8 * (k & 3)); }

// A run of n bytes that a workgroup of kThreads has assembled in LDS (S, dword array, spare dwords behind the run) goes to dst, which
// may have any alignment: the head up to the first 16-byte boundary and the tail by bytes, the body as aligned 16-byte stores whose
// dwords are taken from the LDS dwords at the matching offset with v_alignbyte_b32 (the discipline of convert.hip's staged stores).
template <int kThreads> __device__ __forceinline__ void flush_run(const uint32_t* S, uint8_t* dst, uint32_t n, uint32_t tid)
{
    const uint32_t head = min(n, (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u));
    if (tid < head) dst[tid] = (uint8_t)byte_of(S, tid);
    const uint32_t chunks = (n - head) >> 4;
    for (uint32_t c = tid; c < chunks; c += kThreads) {
        const uint32_t r = head + 16u * c, i = r >> 2, sh = r & 3u;
        const uint32_t a0 = S[i], a1 = S[i + 1], a2 = S[i + 2], a3 = S[i + 3], a4 = S[i + 4];
        *reinterpret_cast<uint4*>(dst + r) = make_uint4(__builtin_amdgcn_alignbyte(a1, a0, sh), __builtin_amdgcn_alignbyte(a2, a1, sh),
                                                        __builtin_amdgcn_alignbyte(a3, a2, sh), __builtin_amdgcn_alignbyte(a4, a3, sh));
    }
    const uint32_t t = head + 16u * chunks + tid;
    if (t < n) dst[t] = (uint8_t)byte_of(S, t);
}

} // namespace gamut
