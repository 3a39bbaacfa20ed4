// png_file.hpp -- the PNG file on the host (png_file.hip): the chunk walk, the zlib inflate, the rules of the reference that the
// callers of both would otherwise each restate, and the arithmetic of the sliced IDAT upload.  No kernel, no stream: what is here
// runs without a GPU (tests/c/png_host_check.cpp); HostBuf's page-locked allocation is the only HIP call.
#pragma once
#include "common.hpp"
#include <utility>

namespace gamut {

using IdatSegments = std::vector<std::pair<const uint8_t*, uint32_t>>;      // the payloads of a file's IDAT chunks, where they lie in the file

struct PngHeader {
    uint32_t x = 0, y = 0; int depth = 0, color = 0, interlace = 0, img_n = 0, pal_img_n = 0;
    bool has_trans = false, is_iphone = false;
    uint8_t palette[1024] = {}; uint32_t pal_len = 0;     // zero-initialised like the D array (stbdec.d:1779): indices >= pal_len expand to (0,0,0,0)
    uint16_t tc[3] = { 0, 0, 0 };      // tRNS key: 8-bit values already scaled (stbdec.d:1945), 16-bit as-is (:1941)
    float ppmX = -1, ppmY = -1, aspect = -1;
    uint8_t* idata = nullptr; uint32_t ioff = 0;
    // the batch path that inflates on the GPU gathers the IDAT payloads itself, slice by slice: parse() then only notes where they are
    IdatSegments* idat_segments = nullptr;
    bool seen_idat = false;
    ~PngHeader() { free(idata); }

    // bytes of a row of the inflated stream without its filter byte (img_width_bytes of stbi__create_png_image_raw, stbdec.d:1424)
    uint64_t row_bytes() const { return ((uint64_t)img_n * x * (uint32_t)depth + 7) >> 3; }
    // what the de-filter of a non-interlaced image reads: a filter byte and a row, y times (img_len, :1425)
    uint64_t defilter_bytes() const { return (row_bytes() + 1) * y; }
    // room for the inflated stream in the device arena.  Adam7: <= 15/8 y rows, each with a filter byte and a rounded-up last byte
    uint64_t slot_bytes() const { return (row_bytes() + 8) * y + 64; }
    // bits per sample as decoded (stbdec.d:669-707 convert from there)
    int bits() const { return depth <= 8 ? 8 : 16; }
};
constexpr uint64_t kMaxSlotBytes = 0xFFFFFF00ull;          // a larger slot_bytes(): "png: image too large" (stream lengths are 32-bit)

// channels of the de-filtered image for a caller that asks for req_comp (stbdec.d:1821-1824)
inline int png_out_channels(const PngHeader& h, int req_comp)
{
    return ((req_comp == h.img_n + 1 && req_comp != 3 && !h.pal_img_n) || h.has_trans) ? h.img_n + 1 : h.img_n;
}
// the two bytes in front of a DEFLATE stream (stbi__parse_zlib_header, stbdec.d:1281-1290); that there ARE two is the caller's to check
inline bool zlib_header_ok(uint8_t b0, uint8_t b1) { return ((b0 * 256 + b1) % 31) == 0 && !(b1 & 32) && (b0 & 15) == 8; }

// header_only: stop as stbi__png_info_raw does (SCAN_header), enough for stbi__png_is16
int parse(const uint8_t* data, size_t len, PngHeader& h, bool header_only);

// Where zlib writes the inflated stream.  Page-locked (the per-thread staging of the single-image calls: the upload is
// then a plain DMA -- an upload from freshly written pageable memory was seen to take 12-22 ms for 4 MB on some boxes,
// 0.2 ms on others; intentionally not freed at thread exit, the HIP runtime may already be gone) or plain malloc memory
// (the short-lived worker threads of the batch call).
struct HostBuf {
    uint8_t* p = nullptr; size_t cap = 0; bool pinned = false;
    bool reserve(size_t n, size_t keep);
    void release() { if (p) { if (pinned) (void)hipHostFree(p); else free(p); } p = nullptr; cap = 0; }
};

// stbi_zlib_decode_malloc_guesssize_headerflag (stbdec.d:1267-1321); the result lives in `out` (not to be freed)
uint8_t* inflate_idat(const uint8_t* buf, uint32_t len, size_t guess, uint32_t* outlen, bool parse_header, HostBuf& out);

// parse + inflate of one file (host only)
struct PngJob { PngHeader h; HostBuf raw; uint32_t raw_len = 0; int rc = GAMUT_HIP_OK; char msg[160] = { 0 }; };
int png_prepare(const uint8_t* data, size_t len, PngJob& j);

// What the batch call knows of one file once its host stage is through.
struct BatchFile {
    int rc = GAMUT_HIP_OK; char msg[160] = { 0 };
    bool uploaded = false, batched = false;   // inflated stream in the device arena; de-filter goes into a batched launch
    PngHeader h;                      // (idata released)
    uint32_t raw_len = 0, need = 0; int out_n = 0, bits = 8, channels_in_file = 0;

    void fail(int index, int code, const char* text) { rc = code; snprintf(msg, sizeof(msg), "image %d: %s", index, text); }
    // the header is known: what the later stages read from it
    void accept(const PngHeader& header, int req_comp)
    {
        h = header;
        out_n = png_out_channels(h, req_comp); bits = h.bits(); channels_in_file = h.img_n;
        need = (uint32_t)h.defilter_bytes();
    }
};
// Files that need nothing but de-filter + expand -- not interlaced, no palette, no tRNS, channel count and depth as asked, the whole
// stream there -- are de-filtered together, one launch per geometry; the others run the whole of stbi__do_png on their own.
inline bool batched(const BatchFile& f, int req_comp, int bits)
{
    return !f.h.interlace && !f.h.has_trans && !f.h.pal_img_n && (req_comp == 0 || req_comp == f.out_n) && (bits == 0 || bits == f.bits) && f.raw_len >= f.need;
}

// ---- the sliced upload of the device inflate -------------------------------------------------------------------------------
// The IDAT bytes of the batch go up SLICE BY SLICE -- slice r of every stream, then slice r + 1 of every stream -- and the inflate
// kernel is launched once per slice behind them.  The plan is arithmetic only: which streams, in which order, how long a slice, how
// the staging image is laid out, which (round, stream) units of copying there are.
struct SliceOverrides {
    uint32_t slice = 0;               // bytes, 0: the plan's own choice (GAMUT_HIP_PNG_SLICE_KB; still doubled until 32 rounds suffice)
    int pitched = -1;                 // 0 / 1: force the layout (GAMUT_HIP_PNG_PITCHED); -1: the plan's own choice
};
struct SlicePlan {
    std::vector<int> who;             // the streams (file indices), longest first; k below is a position in this list
    std::vector<uint32_t> len;        // len[k]: bytes of stream who[k]
    uint32_t slice = 0; int rounds = 1;
    uint64_t pitch = 0; bool pitched = false;          // pitched: stream k's share of the image starts at k * pitch; else the shares lie tight
    uint64_t blob_bytes = 0; std::vector<uint64_t> blob_off;      // blob_off[file]: where the file's share starts (files not in `who`: 0)
    std::vector<std::pair<int, int>> units;            // (round r, k), round-major: copy bytes [r * slice, ...) of stream k into its share
    std::vector<int> units_in_round;                   // the streams of round r are who[0 .. units_in_round[r])
    // bytes of stream k that are in the image once round r has gone up
    uint32_t avail(int r, size_t k) const { return (uint32_t)std::min<uint64_t>((uint64_t)(r + 1) * slice, len[k]); }
};
// idat_len / slot_bytes per file of the batch (slot_bytes: the room for the file's inflated stream); streams: the files that take part
SlicePlan plan_slices(const std::vector<uint32_t>& idat_len, const std::vector<int64_t>& slot_bytes, const std::vector<int>& streams, const SliceOverrides& overrides);

// bytes [lo, hi) of a file's zlib stream = bytes [lo + skip, hi + skip) of its concatenated IDAT payloads, copied to dst
void copy_idat_range(const IdatSegments& segments, uint32_t skip, uint64_t lo, uint64_t hi, uint8_t* dst);

} // namespace gamut
