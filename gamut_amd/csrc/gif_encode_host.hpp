// gif_encode_host.hpp -- what gif_encode.hip (the kernels) and gif_encode_host.hip (arguments, tables, entry points) share.
#pragma once
#include "common.hpp"

namespace gamut {

struct GifEncAnim {                      // one animation of the batch (device table)
    const uint8_t* src;                  // layer 0, row 0
    int64_t  pitch, layer_off, out_off;
    uint32_t w, h, frames, frame0;       // frame0: index of its first frame in the batch's frame tables
    int32_t  centis, max_depth, alpha_thr;
    uint32_t aligned;                    // src, pitch and layer_off are all multiples of 4: pixels are fetched as dwords
};
struct GifEncFrame {                     // one frame of the batch (device table, written by the host)
    uint64_t slot;                       // byte offset of the frame's block slot in the slot scratch, a multiple of 4
    uint32_t slot_cap;                   // bytes the block may take (the reference's reservation); the slot holds 3 more
    uint32_t anim, index;                // whose frame, which one
    uint32_t census0, gather0;           // first workgroup of the frame in the census / gather grids
    uint32_t pad;
};
struct GifEncPlan {                      // per frame, written by k_gifenc_plan and k_gifenc_lzw
    int32_t  depth, count, has_transparent, compatible;
    uint32_t block_len;                  // bytes of the frame's block (GCE .. terminator)
    uint32_t block_pad;                  // the block starts this many bytes into its slot
    uint32_t overflow;                   // a store was dropped at the slot's end (cannot happen within the reference's reservation)
    uint32_t resv;
    uint64_t file_off;                   // where the block starts in its file (k_gifenc_offsets)
};
struct GifEncMul {                       // the rmul / gmul / bmul constant by channel bits 0..6 (msf_gif.d:214-216), made on the host: 9 bits each
    uint64_t packed;
    __host__ __device__ uint32_t of(int bits) const { return (uint32_t)(packed >> (9 * bits)) & 511u; }
};

constexpr uint32_t kGifCensusWords  = 4100;     // the used-value bitmaps of depths 1..16 of one frame, 32-bit words (depth d at gifenc_bitmap_word(d))
constexpr uint32_t kGifCensusPixels = 8192;     // pixels per census workgroup
constexpr uint32_t kGifGatherBytes  = 4096;     // block bytes per gather workgroup

int64_t gifenc_frame_reservation(int w, int h);                     // msf_gif.d:337-345
int64_t gifenc_bound(int w, int h, int frames);                     // 0 when refused
GifEncMul gifenc_mul_table();

// gif_encode.hip: the five launches of one call, asynchronous on `stream`, with the timer's 6 marks around them
int gifenc_launch(const GifEncAnim* anims, int n_anim, const GifEncFrame* frames, uint32_t n_frames, uint32_t census_units, uint32_t gather_units,
                  uint32_t* bitmaps, uint32_t* transp, GifEncPlan* plans, uint8_t* slots, int64_t* total_len, uint8_t* out, const GifEncMul& mul,
                  hipStream_t stream, KernelTimer<6>& timer);

} // namespace gamut
