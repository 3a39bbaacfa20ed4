// encode_host.hpp -- what the host drop-ins that encode ONE image share (qoi_encode, jpeg_encode, png / bmp / gif / tga _write_to_mem).
#pragma once
#include "common.hpp"

namespace gamut {

// runtime.hip: the calling thread's staging for a single-image encode on the current device, ONE pair of buffers whatever the codec
// (grown on demand, never shrunk): device_bytes of HBM are returned, *pinned (asked for only when `pinned` is given) gets pinned_bytes
// of page-locked memory.  NULL when either cannot be had.
uint8_t* encode_staging(size_t device_bytes, size_t pinned_bytes, hipStream_t stream, uint8_t** pinned);

struct HostRows { const void* base; int64_t pitch; size_t row_bytes; int rows; int layers; int64_t layer_offset; };   // pitch may be negative

// The pixels go up through pinned staging, rows and layers packed; `encode` is the codec's batch call on a batch of one,
//   int encode(const uint8_t* device_src, int64_t tight_pitch, int64_t tight_layer, int64_t out_offset, uint8_t* device_base, int64_t* len, hipStream_t)
// which writes at most `bound` bytes at device_base + out_offset and returns the call's status; the stream comes back in malloc
// memory (*out_len bytes), or NULL with the thread's message, which starts with `name`.  The thread's stream is waited for on every
// way out behind the upload: the pinned buffer the DMA reads belongs to the thread's next call, another codec's perhaps.
template <class Encode>
void* encode_host_image(const char* name, const HostRows& src, size_t bound, int* out_len, Encode encode)
{
    const size_t row = src.row_bytes, layer = row * (size_t)src.rows, px_bytes = layer * (size_t)src.layers, o_out = up256(px_bytes);
    hipStream_t st = thread_stream();
    uint8_t* h = nullptr;
    uint8_t* d = encode_staging(o_out + bound, px_bytes, st, &h);
    if (!d) { set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "%s: staging of %zu bytes failed", name, o_out + bound); return nullptr; }
    for (int l = 0; l < src.layers; ++l)
        for (int y = 0; y < src.rows; ++y)
            memcpy(h + layer * l + row * y, static_cast<const uint8_t*>(src.base) + (ptrdiff_t)src.layer_offset * l + (ptrdiff_t)src.pitch * y, row);
    int rc; int64_t n = 0;
    if (hipMemcpyAsync(d, h, px_bytes, hipMemcpyHostToDevice, st) != hipSuccess) { (void)hipGetLastError(); rc = set_error(GAMUT_HIP_ERR_HIP, "%s: upload failed", name); }
    else {
        try { rc = encode(d, (int64_t)row, (int64_t)layer, (int64_t)o_out, d, &n, st); }
        catch (...) { rc = set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "%s: out of host memory", name); }
    }
    void* result = nullptr;
    if (rc == GAMUT_HIP_OK && !(result = malloc((size_t)n))) set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "%s: out of memory", name);
    const bool copied = result && hipMemcpyAsync(result, d + o_out, (size_t)n, hipMemcpyDeviceToHost, st) == hipSuccess;
    const bool drained = hipStreamSynchronize(st) == hipSuccess;
    if (result && !(copied && drained)) { (void)hipGetLastError(); free(result); result = nullptr; set_error(GAMUT_HIP_ERR_HIP, "%s: copy back failed", name); }
    if (result) *out_len = (int)n;
    return result;
}

} // namespace gamut
