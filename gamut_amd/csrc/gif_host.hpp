// gif_host.hpp -- what the host's walk over a GIF file (gif_host.hip) hands to the batch decoder (gif.hip).
#pragma once
#include "common.hpp"

namespace gamut {

struct GifFrame {
    int32_t fx, fy;                  // frameX, frameY
    int32_t fw;                      // max(frameW, 1): the stream's row length
    int32_t rows;                    // stream rows that land on the screen (a prefix of the stream); rows * fw indices are worth keeping
    int32_t dispose;                 // 0 / 2: what happens to the canvas BEFORE this frame (0 for the first frame)
    int32_t pal;                     // which of the file's palette snapshots
    int32_t lzw_cs;
    int64_t rowmap;                  // interlaced: offset of `height` entries in rowmaps (screen row -> stream row, 0xFFFF: none); -1: stream row = y - fy
    size_t  payload_off, payload_len;
};
struct GifParsed {                   // one file
    std::vector<GifFrame> frames;
    std::vector<uint8_t>  payload;   // every frame's sub-block chain in one piece, frame after frame
    std::vector<uint32_t> palettes;  // snapshots of 256 (R, G, B, A) words, a new one only where the current palette changed
    std::vector<uint16_t> rowmaps;
};

// walk_codes: the first pass walks every LZW code (the whole verdict of GIFDecoder.open); otherwise only the sub-block chains.
// out == nullptr: the first pass alone.  info is zeroed (pixel_aspect_ratio -1) when the file is refused.
int gif_parse(const uint8_t* data, size_t len, bool walk_codes, GifParsed* out, gamut_hip_gif_info* info);

} // namespace gamut
