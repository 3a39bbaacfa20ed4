// tga_host.hip -- the TGA header on the host: TGADecoder.getImageInfo plus the header-level part of decodeImage
// (source/gamut/codecs/tga.d:313-382, 384-417, 601-623) restated, so that gamut_hip_tga_read_header gives the reference's
// two verdicts on a file without touching a GPU.
//
// The reference reads through a memory stream (io.d mread / mseek): a read past the end FAILS (it does not hand out zeros, as
// the BMP reader does), a skip to exactly the end succeeds and one byte further fails.
//
// DETECT (detectTGA, plugins/tga.d:97-126) is getImageInfo alone, bytes 0..16: info->detected.  It is what identification
// asks.  LOAD adds the descriptor byte (byte 17; bit 5 clear means the first row in the file is the bottom one), the skip of
// the ID field, the components and rgb16 flag of stbi__tga_get_comp and the size test: the return value.  A file of 17 bytes
// can be detected and not loaded.
//
// Kept from the reference: the colour-map fields are only read when cmapType is 1 (a type 2 file's are skipped and stay 0);
// the components come from the cmap size when indexed and from bpp otherwise (bpp 8 gives one component even for type 2, 16-bit
// grey gives two, 15 / 16 bits otherwise give rgb16 and three); the descriptor's alpha bits and x-origin bit are ignored.
//
// DELIBERATE DEVIATION: width * height * components > 2^31 - 1 is refused.  The reference indexes its pixels with `int`
// (tga.d:427, :473, :549), which wraps there.  (GAMUT_MAX_IMAGE_BYTES and imageIsValidSize cannot fail for 16-bit dimensions.)
#include "common.hpp"

namespace gamut {
namespace {

struct MemReader {                                                 // io.d: read_ubyte / read_ushort_LE / skipBytes on a MemoryFile
    const uint8_t* p; size_t len; size_t pos = 0; bool err = false;
    uint32_t get8() { if (pos < len) return p[pos++]; err = true; return 0; }
    uint32_t get16() { if (len - pos >= 2) { const uint32_t v = p[pos] | (uint32_t)p[pos + 1] << 8; pos += 2; return v; } err = true; return 0; }
    bool skip(size_t n) { if (n <= len - pos) { pos += n; return true; } return false; }          // mseek: up to and including the end
};

} // namespace

int tga_fail(const char* why) { return set_error(GAMUT_HIP_ERR_DECODE, "tga: %s", why); }

// stbi__tga_get_comp :601-623
int tga_get_comp(int bits, bool is_grey, int* rgb16)
{
    *rgb16 = 0;
    switch (bits) {
    case 8: return 1;
    case 16: if (is_grey) return 2; /* fallthrough */
    case 15: *rgb16 = 1; return 3;
    case 24: case 32: return bits / 8;
    default: return 0;
    }
}

int tga_parse_header(const uint8_t* data, size_t len, gamut_hip_tga_info* info)
{
    memset(info, 0, sizeof(*info));
    MemReader s{ data, data ? len : 0 };
    // ---- getImageInfo :313-382
    const uint32_t id_len = s.get8();
    if (s.err) return tga_fail("no header");
    const uint32_t cmap_type = s.get8();
    if (s.err || cmap_type > 1) return tga_fail("colour map type above 1");
    uint32_t type = s.get8();
    if (s.err) return tga_fail("short header");
    uint32_t pal_start = 0, pal_len = 0, cmap_size = 0;
    if (cmap_type == 1) {
        if (type != 1 && type != 9) return tga_fail("colour map with an image type other than 1 / 9");
        pal_start = s.get16(); if (s.err) return tga_fail("short header");
        pal_len = s.get16(); if (s.err) return tga_fail("short header");
        if (pal_len == 0) return tga_fail("empty colour map");
        cmap_size = s.get8(); if (s.err) return tga_fail("short header");
        if (cmap_size != 8 && cmap_size != 15 && cmap_size != 16 && cmap_size != 24 && cmap_size != 32) return tga_fail("bad colour map entry size");
        if (!s.skip(4)) return tga_fail("short header");
    } else {
        if (type != 2 && type != 3 && type != 10 && type != 11) return tga_fail("bad image type");
        if (!s.skip(9)) return tga_fail("short header");
    }
    const uint32_t w = s.get16(); if (s.err) return tga_fail("short header");
    const uint32_t h = s.get16(); if (s.err) return tga_fail("short header");
    if (w < 1 || h < 1) return tga_fail("zero width or height");
    const uint32_t bpp = s.get8(); if (s.err) return tga_fail("short header");
    if (cmap_type == 1 && bpp != 8 && bpp != 16) return tga_fail("index size other than 8 / 16 bits");
    if (bpp != 8 && bpp != 15 && bpp != 16 && bpp != 24 && bpp != 32) return tga_fail("bad bits per pixel");
    info->detected = 1;
    info->width = (int32_t)w; info->height = (int32_t)h; info->bpp = (int32_t)bpp;
    info->indexed = (int32_t)cmap_type; info->palette_start = (int32_t)pal_start; info->palette_len = (int32_t)pal_len; info->cmap_size = (int32_t)cmap_size;
    // ---- decodeImage :384-417
    info->rle = type >= 8;
    if (type >= 8) type -= 8;
    info->image_type = (int32_t)type;
    const uint32_t desc = s.get8();
    if (s.err) return tga_fail("no descriptor byte");
    info->bottom_up = 1 - (int32_t)((desc >> 5) & 1u);
    info->channels_in_file = cmap_type ? tga_get_comp((int)cmap_size, false, &info->rgb16) : tga_get_comp((int)bpp, type == 3, &info->rgb16);
    if (!s.skip(id_len)) return tga_fail("ID field past the end");
    info->data_offset = (int32_t)s.pos;
    if ((uint64_t)w * h * (uint32_t)info->channels_in_file > 0x7fffffffull) return tga_fail("too large");                  // DEVIATION
    return GAMUT_HIP_OK;
}

} // namespace gamut

using namespace gamut;

extern "C" int gamut_hip_tga_read_header(const uint8_t* data, size_t len, gamut_hip_tga_info* info)
{
    clear_error();
    if (!info) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "tga_read_header: info is NULL");
    return tga_parse_header(data, len, info);
}
