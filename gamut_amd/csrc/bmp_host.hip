// bmp_host.hip -- the BMP header on the host: stbi__bmp_parse_header plus the header-level part of stbi__bmp_load
// (source/gamut/codecs/stbdec.d:2147-2239, 2270-2345, 2386-2408) restated, so that gamut_hip_bmp_read_header gives the
// reference's verdict on a file without touching a GPU.
//
// The reference's reader hands out 0 for every byte past the end of its input and never rejects a short file (stbi__get8);
// header fields past `len` therefore read as zero here (and pixel bytes past `len` read as zero in bmp.hip).
// bytes_read_so_far (:2297) is the number of header bytes consumed, 14 + header size (+ 12 for the three masks of a 40 / 56
// header), as for a header that lies wholly inside the input.
//
// Where the pixels start.  Palette files (bpp < 16): at bfOffBits.  Files of 16 / 24 / 32 bits: the reference skips to
// bfOffBits (:2310) and then skips bfOffBits - header bytes AGAIN (:2389), so its pixels start at 2 * bfOffBits - header
// bytes; for the usual file (bfOffBits == header bytes) the two are the same place.  info->pixel_offset is where the
// reference reads, and the kernel reads there.
//
// DELIBERATE DEVIATIONS from the reference:
//   * a negative palette size (bfOffBits in front of the palette), where the reference runs stbi__skip with a negative count:
//     refused;
//   * width or height 0 (the reference returns a zero-byte allocation): refused;
//   * a palette index >= the palette size reads uninitialised stack memory in the reference (pal[] :2267); in bmp.hip it
//     reads (0, 0, 0).
#include "common.hpp"

namespace gamut {
namespace {

struct Reader {                                                    // stbi__get8 / get16le / get32le on a memory buffer
    const uint8_t* p; size_t len; size_t pos = 0;
    uint32_t get8() { const uint32_t v = (p && pos < len) ? p[pos] : 0u; ++pos; return v; }
    uint32_t get16() { const uint32_t a = get8(); return a | get8() << 8; }
    uint32_t get32() { const uint32_t a = get16(); return a | get16() << 16; }
};

int high_bit(uint32_t z) { int n = -1; while (z) { ++n; z >>= 1; } return n; }            // stbi__high_bit :2468
int bitcount(uint32_t a) { int n = 0; while (a) { n += a & 1u; a >>= 1; } return n; }     // stbi__bitcount :2480

} // namespace

int bmp_fail(const char* why) { return set_error(GAMUT_HIP_ERR_DECODE, "bmp: %s", why); }

// req_comp decides the decoder's target channel count, which the size test (:2324) is about
int bmp_parse_header(const uint8_t* data, size_t len, int req_comp, gamut_hip_bmp_info* info)
{
    memset(info, 0, sizeof(*info));
    info->pixels_per_meter_x = info->pixels_per_meter_y = info->pixel_aspect_ratio = -1.0f;
    Reader s{ data, data ? len : 0 };
    // ---- stbi__bmp_parse_header :2147-2239
    if (s.get8() != 'B' || s.get8() != 'M') return bmp_fail("not a BMP");
    s.get32(); s.get16(); s.get16();
    const int offset = (int)s.get32();
    const int hsz = (int)s.get32();
    uint32_t mr = 0, mg = 0, mb = 0, ma = 0;
    int extra_read = 14, compress = 0;
    if (offset < 0) return bmp_fail("bad offset");
    if (hsz != 12 && hsz != 40 && hsz != 56 && hsz != 108 && hsz != 124) return bmp_fail("unknown header size");
    uint32_t img_x, img_y;
    if (hsz == 12) { img_x = s.get16(); img_y = s.get16(); }
    else { img_x = s.get32(); img_y = s.get32(); }
    if (s.get16() != 1) return bmp_fail("bad plane count");
    const int bpp = (int)s.get16();
    float ppmX = -1, ppmY = -1, ratio = -1;
    auto mask_defaults = [&] {                                      // stbi__bmp_set_mask_defaults :2121, compress == 0
        if (bpp == 16) { mr = 31u << 10; mg = 31u << 5; mb = 31u; }
        else if (bpp == 32) { mr = 0xffu << 16; mg = 0xffu << 8; mb = 0xffu; ma = 0xffu << 24; }
        else mr = mg = mb = ma = 0;
    };
    if (hsz != 12) {
        compress = (int)s.get32();
        if (compress == 1 || compress == 2) return bmp_fail("RLE is not supported");
        if (compress >= 4) return bmp_fail("unsupported compression");
        // (a NEGATIVE value passes the three tests above in the reference too: it is then refused at :2213 for 16 / 32 bits under a
        //  40 / 56 header, leaves the V4 / V5 masks as the file has them -- set_mask_defaults fails, unheeded -- and is otherwise ignored)
        if (compress == 3 && bpp != 16 && bpp != 32) return bmp_fail("bitfields need 16 or 32 bits per pixel");
        s.get32();
        const int xppm = (int)s.get32(), yppm = (int)s.get32();
        if (xppm > 1) ppmX = (float)xppm;
        if (yppm > 1) ppmY = (float)yppm;
        if (ppmX != -1 && ppmY != -1) ratio = ppmX / ppmY;
        s.get32(); s.get32();
        if (hsz == 40 || hsz == 56) {
            if (hsz == 56) { s.get32(); s.get32(); s.get32(); s.get32(); }
            if (bpp == 16 || bpp == 32) {
                if (compress == 0) mask_defaults();
                else if (compress != 3) return bmp_fail("unsupported compression");
                else {
                    mr = s.get32(); mg = s.get32(); mb = s.get32();
                    extra_read += 12;
                    if (mr == mg && mg == mb) return bmp_fail("equal colour masks");
                }
            }
        } else {
            mr = s.get32(); mg = s.get32(); mb = s.get32(); ma = s.get32();
            if (compress == 0) mask_defaults();
            for (int i = 0; i < 13; ++i) s.get32();
            if (hsz == 124) for (int i = 0; i < 4; ++i) s.get32();
        }
    }
    // ---- stbi__bmp_load :2270-2345
    const bool flip = (int)img_y > 0;
    if ((int)img_y < 0) img_y = 0u - img_y;                         // abs_int; INT_MIN stays 0x80000000 and fails the next test
    if (img_y > (1u << 24) || img_x > (1u << 24)) return bmp_fail("too large");
    if (img_x == 0 || img_y == 0) return bmp_fail("zero width or height");                  // DEVIATION
    int psize = 0;
    if (hsz == 12) { if (bpp < 24) psize = (offset - extra_read - 24) / 3; }
    else if (bpp < 16) psize = (offset - extra_read - hsz) >> 2;
    if (psize < 0) return bmp_fail("offset in front of the palette");                       // DEVIATION
    const int header_bytes = (int)s.pos;                             // == extra_read + hsz
    int pixel_offset = offset;
    if (psize == 0) {
        if (offset < header_bytes || offset - header_bytes > 1024) return bmp_fail("bad offset");
        if (bpp >= 16) pixel_offset = 2 * offset - header_bytes;    // :2310 and :2389 both skip
    }
    const int img_n = (bpp == 24 && ma == 0xff000000u) ? 3 : (ma ? 4 : 3);
    if (bpp < 16) {
        if (psize == 0 || psize > 256) return bmp_fail("bad palette size");
        if (bpp != 1 && bpp != 4 && bpp != 8) return bmp_fail("bad bits per pixel");
    } else {
        const bool easy = bpp == 24 || (bpp == 32 && mb == 0xffu && mg == 0xff00u && mr == 0x00ff0000u && ma == 0xff000000u);
        if (!easy) {
            if (!mr || !mg || !mb) return bmp_fail("bad masks");
            if (bitcount(mr) > 8 || bitcount(mg) > 8 || bitcount(mb) > 8 || bitcount(ma) > 8) return bmp_fail("mask wider than 8 bits");
        }
    }
    const int target = req_comp >= 3 ? req_comp : img_n;
    if ((int64_t)target * img_x > 0x7fffffffLL / img_y) return bmp_fail("too large");        // stbi__mad3sizes_valid(target, x, y, 0) :2324
    info->width = (int32_t)img_x; info->height = (int32_t)img_y; info->bpp = bpp; info->header_size = hsz; info->compression = compress;
    info->channels_in_file = img_n; info->top_down = flip ? 0 : 1; info->pixel_offset = pixel_offset; info->palette_size = psize;
    info->mask_r = mr; info->mask_g = mg; info->mask_b = mb; info->mask_a = ma;
    info->pixels_per_meter_x = ppmX; info->pixels_per_meter_y = ppmY; info->pixel_aspect_ratio = ratio;
    return GAMUT_HIP_OK;
}

} // namespace gamut

using namespace gamut;

// the size test for the file's own channel count (req_comp 0)
extern "C" int gamut_hip_bmp_read_header(const uint8_t* data, size_t len, gamut_hip_bmp_info* info)
{
    clear_error();
    if (!info) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "bmp_read_header: info is NULL");
    return bmp_parse_header(data, len, 0, info);
}
