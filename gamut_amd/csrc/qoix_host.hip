// qoix_host.hip -- the QOIX header on the host: what qoix_lz4_decode (source/gamut/plugins/qoix.d:350-473) and the header part of
// qoix_decode (source/gamut/codecs/qoi2avg.d:634-666) decide before a body byte is looked at, so that gamut_hip_qoix_read_header
// gives the load's verdict without touching a GPU.
//
// The header is 25 bytes: "qoix", width and height (big-endian u32), version (byte 12), channels (13), bitdepth (14), colorspace (15),
// compression (16), pixel aspect ratio and vertical DPI (big-endian floats, bytes 17..24).  With compression 1 a big-endian `orig`
// follows (bytes 25..28) and an LZ4 block that inflates to exactly `orig` bytes; the sub-codec then sees header + orig bytes.
//
// The container's own checks come first (qoix.d:356-391, :412-418, identifyTypeFromStream :476-507): size >= 25, channels 1..4,
// bitdepth 8 or 10, compression 0 or 1, and with compression 1 size >= 29 and orig >= 0 as an int.  The container does NOT test the
// signature; only the sub-codec does.  Then the codec is chosen: 8-bit with 3 or 4 channels is QOI2AVG, the one built here; everything
// else the container accepts is GAMUT_HIP_ERR_UNSUPPORTED.  Then QOI2AVG's header checks (qoi2avg.d:634-666) on the size the sub-codec
// sees: size >= 29, width and height non-zero, colorspace <= 2, version <= 1, the signature, height < 400000000 / width (unsigned).
//
// 8-bit files with 1 or 2 channels are QOI-Plane (source/gamut/codecs/qoiplane.d), built behind the process-wide switch
// gamut_hip_qoix_set_plane (initial value GAMUT_HIP_QOIX_PLANE=0|1, default 0).  Off, they are GAMUT_HIP_ERR_UNSUPPORTED as before the
// codec existed; on, they go through qoiplane_decode's own checks (qoiplane.d:379-411), which are QOI2AVG's with colorspace <= 1: a
// colorspace-2 file with 2 channels is typed lap8 by the container and then refused by the sub-codec.
//
// An early refusal that the reference does not have, and that never changes a verdict: an LZ4 block of n bytes cannot produce more
// than 255 * n bytes.  Proof, per input byte: a literal yields itself (1 byte); a length-extension byte adds at most 255 to a
// literal or match length (255 bytes, and the literal ones need their own input bytes on top); a token yields at most its 15 + 4
// match bytes without extension, and needs two offset bytes besides (19 bytes from 3).  So orig > 255 * (size - 29) can only end in
// "input exhausted" (deviation 1 of qoix.hip), and is refused here before any scratch is sized from the claim.
// tests/test_qoix_cpu.py asserts that this test never disagrees with the restatement.
#include "common.hpp"
#include <atomic>
#include <climits>

namespace gamut {

static std::atomic<int>& plane_switch()
{
    static std::atomic<int> on{ [] { const char* e = getenv("GAMUT_HIP_QOIX_PLANE"); return e && e[0] == '1' && !e[1] ? 1 : 0; }() };
    return on;
}
bool qoix_plane_on() { return plane_switch().load(std::memory_order_relaxed) != 0; }

int qoix_fail(const char* why) { return set_error(GAMUT_HIP_ERR_DECODE, "qoix: %s", why); }

static uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// *sub_size: the `size` qoix_decode is called with (the file's length, or 25 + orig)
int qoix_parse_header(const uint8_t* data, size_t len, gamut_hip_qoix_info* info, uint32_t* sub_size)
{
    memset(info, 0, sizeof(*info));
    info->pixel_type = -1;
    if (sub_size) *sub_size = 0;
    if (!data) len = 0;
    info->detected = len >= 4 && !memcmp(data, "qoix", 4);                      // detectQOIX qoix.d:149-153
    if (len > (size_t)INT_MAX) return qoix_fail("file of more than 2^31 - 1 bytes");          // loadQOIX keeps the length in an int :76
    if (len < 25) return qoix_fail("shorter than the 25-byte header");         // :356
    info->width = (int32_t)be32(data + 4); info->height = (int32_t)be32(data + 8);
    info->version = data[12]; info->channels = data[13]; info->bitdepth = data[14]; info->colorspace = data[15]; info->compression = data[16];
    const uint32_t par = be32(data + 17), dpi = be32(data + 21);               // qoi_read_32f: the bits as they are
    memcpy(&info->pixel_aspect_ratio, &par, 4); memcpy(&info->resolution_y, &dpi, 4);
    const int ch = info->channels, depth = info->bitdepth;
    if (ch < 1 || ch > 4 || (depth != 8 && depth != 10)) return qoix_fail("channels outside 1..4 or a bit depth other than 8 / 10");   // :476-507
    const bool premul = info->colorspace == 2;                                  // :367
    static const int t8[5] = { -1, GAMUT_PIXEL_l8, GAMUT_PIXEL_la8, GAMUT_PIXEL_rgb8, GAMUT_PIXEL_rgba8 };
    static const int t16[5] = { -1, GAMUT_PIXEL_l16, GAMUT_PIXEL_la16, GAMUT_PIXEL_rgb16, GAMUT_PIXEL_rgba16 };
    int type = depth == 8 ? t8[ch] : t16[ch];
    if (premul && ch == 2) type = depth == 8 ? GAMUT_PIXEL_lap8 : GAMUT_PIXEL_lap16;
    if (premul && ch == 4) type = depth == 8 ? GAMUT_PIXEL_rgbap8 : GAMUT_PIXEL_rgbap16;
    info->pixel_type = type;
    uint32_t size = (uint32_t)len;
    if (info->compression == 1) {                                               // :381-411
        if (len < 29) return qoix_fail("compressed file shorter than 29 bytes");
        info->orig = (int32_t)be32(data + 25);
        if (info->orig < 0) return qoix_fail("negative original size");
        size = 25u + (uint32_t)info->orig;
    } else if (info->compression != 0) return qoix_fail("compression other than 0 / 1");      // :417-418
    const bool plane = depth == 8 && ch < 3;
    if (depth == 10 || (plane && !qoix_plane_on()))
        return set_error(GAMUT_HIP_ERR_UNSUPPORTED, "qoix: the %d-bit %d-channel codec is not built yet", depth, ch);
    // qoix_decode qoi2avg.d:634-666, qoiplane_decode qoiplane.d:379-411
    if (size < 29) return qoix_fail("no room for the 4 closing bytes");
    const uint32_t w = (uint32_t)info->width, h = (uint32_t)info->height;
    if (w == 0 || h == 0) return qoix_fail("zero width or height");
    if (info->colorspace > (plane ? 1 : 2)) return qoix_fail(plane ? "colorspace above 1 in a QOI-Plane file" : "colorspace above 2");
    if (info->version > 1) return qoix_fail("version above 1");
    if (!info->detected) return qoix_fail("bad signature");
    if (h >= 400000000u / w) return qoix_fail("too many pixels");
    if (info->compression == 1 && (uint64_t)(uint32_t)info->orig > 255ull * (len - 29)) return qoix_fail("original size beyond what the LZ4 block can produce");
    if (sub_size) *sub_size = size;
    return GAMUT_HIP_OK;
}

} // namespace gamut

using namespace gamut;

extern "C" int gamut_hip_qoix_read_header(const uint8_t* data, size_t len, gamut_hip_qoix_info* info)
{
    clear_error();
    if (!info) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "qoix_read_header: info is NULL");
    return qoix_parse_header(data, len, info, nullptr);
}

extern "C" int gamut_hip_qoix_set_plane(int on)
{
    if (on != 0 && on != 1) return plane_switch().load(std::memory_order_relaxed);
    return plane_switch().exchange(on, std::memory_order_relaxed);
}
