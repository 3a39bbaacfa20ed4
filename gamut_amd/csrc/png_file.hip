// png_file.hip -- the PNG file on the host, without a GPU (png_file.hpp).
//
// Host feeder = what stays on the CPU in the reference too:
// the chunk walk of stbi__parse_png_file (stbdec.d:1777-2023: IHDR/PLTE/tRNS/pHYs/CgBI/IDAT,
// missing-IEND tolerance :2008-2012) and the inflate of finalize_decode (:1808-1819; the
// reference calls the third-party `miniz`, here the system zlib in raw mode with the adler32
// unchecked like the reference's trusted_input=true).  Behind them the arithmetic of the batch
// call's sliced IDAT upload (plan_slices, copy_idat_range): pure functions, checked on the CPU
// by tests/c/png_host_check.cpp.
#include "png_file.hpp"
#include <zlib.h>

namespace gamut {
namespace {

struct Reader {                       // stb's memory reader: reads past the end yield 0 (stbi__get8)
    const uint8_t* p; const uint8_t* end;
    int      get8()    { return p < end ? *p++ : 0; }
    uint32_t get16be() { uint32_t z = (uint32_t)get8(); return (z << 8) + (uint32_t)get8(); }
    uint32_t get32be() { uint32_t z = get16be(); return (z << 16) + get16be(); }
    bool     eof() const { return p >= end; }
    void     skip(uint32_t n) { if ((size_t)(end - p) < n) p = end; else p += n; }
};

const uint8_t kDepthScale[9] = { 0, 0xff, 0x55, 0, 0x11, 0, 0, 0, 0x01 };
constexpr uint32_t fourcc(char a, char b, char c, char d) { return ((uint32_t)(uint8_t)a << 24) | ((uint32_t)(uint8_t)b << 16) | ((uint32_t)(uint8_t)c << 8) | (uint8_t)d; }

} // namespace

// header_only: stop as stbi__png_info_raw does (SCAN_header), enough for stbi__png_is16
int parse(const uint8_t* data, size_t len, PngHeader& h, bool header_only)
{
    static const uint8_t sig[8] = { 137, 80, 78, 71, 13, 10, 26, 10 };
    Reader s{ data, data + len };
    for (int i = 0; i < 8; ++i) if (s.get8() != sig[i]) return set_error(GAMUT_HIP_ERR_DECODE, "png: bad signature");
    bool first = true; uint32_t cap = 0;
    for (;;) {
        const uint32_t clen = s.get32be(), type = s.get32be();
        switch (type) {
        case fourcc('C','g','B','I'): h.is_iphone = true; s.skip(clen); break;
        case fourcc('p','H','Y','s'):
            h.ppmX = (float)s.get32be(); h.ppmY = (float)s.get32be(); h.aspect = h.ppmX / h.ppmY;
            if (s.get8() != 1) { h.ppmX = -1; h.ppmY = -1; }
            break;
        case fourcc('I','H','D','R'): {
            if (!first || clen != 13) return set_error(GAMUT_HIP_ERR_DECODE, "png: bad IHDR");
            first = false;
            h.x = s.get32be(); h.y = s.get32be();
            if (h.y > (1u << 24) || h.x > (1u << 24)) return set_error(GAMUT_HIP_ERR_DECODE, "png: too large");
            h.depth = s.get8();
            if (h.depth != 1 && h.depth != 2 && h.depth != 4 && h.depth != 8 && h.depth != 16) return set_error(GAMUT_HIP_ERR_DECODE, "png: 1/2/4/8/16-bit only");
            h.color = s.get8();
            if (h.color > 6 || (h.color == 3 && h.depth == 16)) return set_error(GAMUT_HIP_ERR_DECODE, "png: bad ctype");
            if (h.color == 3) h.pal_img_n = 3; else if (h.color & 1) return set_error(GAMUT_HIP_ERR_DECODE, "png: bad ctype");
            if (s.get8()) return set_error(GAMUT_HIP_ERR_DECODE, "png: bad comp method");
            if (s.get8()) return set_error(GAMUT_HIP_ERR_DECODE, "png: bad filter method");
            h.interlace = s.get8(); if (h.interlace > 1) return set_error(GAMUT_HIP_ERR_DECODE, "png: bad interlace method");
            if (!h.x || !h.y) return set_error(GAMUT_HIP_ERR_DECODE, "png: 0-pixel image");
            if (!h.pal_img_n) {
                h.img_n = (h.color & 2 ? 3 : 1) + (h.color & 4 ? 1 : 0);
                if ((1u << 30) / h.x / (uint32_t)h.img_n < h.y) return set_error(GAMUT_HIP_ERR_DECODE, "png: too large");
                if (header_only) return GAMUT_HIP_OK;
            } else {
                h.img_n = 1;
                if ((1u << 30) / h.x / 4 < h.y) return set_error(GAMUT_HIP_ERR_DECODE, "png: too large");
            }
        } break;
        case fourcc('P','L','T','E'):
            if (first || clen > 256 * 3) return set_error(GAMUT_HIP_ERR_DECODE, "png: invalid PLTE");
            h.pal_len = clen / 3;
            if (h.pal_len * 3 != clen) return set_error(GAMUT_HIP_ERR_DECODE, "png: invalid PLTE");
            for (uint32_t i = 0; i < h.pal_len; ++i) {
                h.palette[i*4] = (uint8_t)s.get8(); h.palette[i*4+1] = (uint8_t)s.get8(); h.palette[i*4+2] = (uint8_t)s.get8(); h.palette[i*4+3] = 255;
            }
            break;
        case fourcc('t','R','N','S'):
            if (first) return set_error(GAMUT_HIP_ERR_DECODE, "png: first not IHDR");
            if (h.idata || h.seen_idat) return set_error(GAMUT_HIP_ERR_DECODE, "png: tRNS after IDAT");
            if (h.pal_img_n) {
                if (header_only) { h.img_n = 4; return GAMUT_HIP_OK; }
                if (h.pal_len == 0 || clen > h.pal_len) return set_error(GAMUT_HIP_ERR_DECODE, "png: bad tRNS");
                h.pal_img_n = 4;
                for (uint32_t i = 0; i < clen; ++i) h.palette[i*4+3] = (uint8_t)s.get8();
            } else {
                if (!(h.img_n & 1) || clen != (uint32_t)h.img_n * 2) return set_error(GAMUT_HIP_ERR_DECODE, "png: bad tRNS");
                h.has_trans = true;
                for (int k = 0; k < h.img_n; ++k) {
                    const uint32_t v = s.get16be();
                    h.tc[k] = h.depth == 16 ? (uint16_t)v : (uint16_t)(uint8_t)((uint8_t)(v & 255) * kDepthScale[h.depth]);
                }
            }
            break;
        case fourcc('I','D','A','T'): {
            if (first) return set_error(GAMUT_HIP_ERR_DECODE, "png: first not IHDR");
            if (h.pal_img_n && !h.pal_len) return set_error(GAMUT_HIP_ERR_DECODE, "png: no PLTE");
            if (header_only) { h.img_n = h.pal_img_n ? h.pal_img_n : h.img_n; return GAMUT_HIP_OK; }
            if ((int32_t)(h.ioff + clen) < (int32_t)h.ioff) return set_error(GAMUT_HIP_ERR_DECODE, "png: IDAT overflow");
            h.seen_idat = true;
            if (h.idat_segments) {
                if ((size_t)(s.end - s.p) < clen) return set_error(GAMUT_HIP_ERR_DECODE, "png: out of data");
                if (clen) h.idat_segments->emplace_back(s.p, clen);
                s.p += clen; h.ioff += clen;
                break;
            }
            if (h.ioff + clen > cap) {
                uint32_t ncap = cap ? cap : (clen > 4096 ? clen : 4096);
                while (h.ioff + clen > ncap) ncap *= 2;
                uint8_t* n = (uint8_t*)realloc(h.idata, ncap);
                if (!n) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "png: out of memory");
                h.idata = n; cap = ncap;
            }
            if ((size_t)(s.end - s.p) < clen) return set_error(GAMUT_HIP_ERR_DECODE, "png: out of data");
            memcpy(h.idata + h.ioff, s.p, clen); s.p += clen; h.ioff += clen;
        } break;
        case fourcc('I','E','N','D'):
            if (first) return set_error(GAMUT_HIP_ERR_DECODE, "png: first not IHDR");
            return GAMUT_HIP_OK;
        default:
            if (first) return set_error(GAMUT_HIP_ERR_DECODE, "png: first not IHDR");
            if (type == 0 && s.eof()) return GAMUT_HIP_OK;                 // Gamut issue #92: no IEND
            if ((type & (1u << 29)) == 0) return set_error(GAMUT_HIP_ERR_DECODE, "png: unknown critical chunk");
            s.skip(clen);
            break;
        }
        s.get32be();      // CRC, not checked
    }
}

bool HostBuf::reserve(size_t n, size_t keep)
{
    if (n <= cap) return true;
    const size_t ncap = n + n / 8 + 4096;
    if (pinned) {
        void* np = nullptr;
        if (hipHostMalloc(&np, ncap, hipHostMallocDefault) != hipSuccess) return false;
        if (keep) memcpy(np, p, keep);
        if (p) (void)hipHostFree(p);
        p = (uint8_t*)np;
    } else {
        uint8_t* np = (uint8_t*)realloc(p, ncap);
        if (!np) return false;
        p = np;
    }
    cap = ncap;
    return true;
}

// stbi_zlib_decode_malloc_guesssize_headerflag (stbdec.d:1267-1321); the result lives in `out` (not to be freed)
uint8_t* inflate_idat(const uint8_t* buf, uint32_t len, size_t guess, uint32_t* outlen, bool parse_header, HostBuf& out)
{
    if (parse_header) {
        if (len < 2 || !zlib_header_ok(buf[0], buf[1])) { set_error(GAMUT_HIP_ERR_DECODE, "png: bad zlib header"); return nullptr; }
        buf += 2; len -= 2;
    }
    size_t cap = guess ? guess : 1;
    z_stream z; memset(&z, 0, sizeof(z));
    if (!out.reserve(cap, 0) || inflateInit2(&z, -15) != Z_OK) { set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "png: inflate init failed"); return nullptr; }
    z.next_in = const_cast<Bytef*>(buf); z.avail_in = len; z.next_out = out.p; z.avail_out = (uInt)cap;
    for (;;) {
        const int r = inflate(&z, Z_NO_FLUSH);
        if (r == Z_STREAM_END) break;
        if ((r == Z_OK || r == Z_BUF_ERROR) && z.avail_out == 0 && cap <= 536870912u) {
            size_t ncap = cap * 2; if (ncap < 32 * 1024) ncap = 32 * 1024;
            if (!out.reserve(ncap, cap)) { inflateEnd(&z); set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "png: out of memory"); return nullptr; }
            z.next_out = out.p + cap; z.avail_out = (uInt)(ncap - cap); cap = ncap;
            continue;
        }
        if (r == Z_OK && z.avail_in != 0) continue;
        inflateEnd(&z); set_error(GAMUT_HIP_ERR_DECODE, "png: corrupt zlib stream"); return nullptr;
    }
    *outlen = (uint32_t)z.total_out;
    inflateEnd(&z);
    return out.p;
}

int png_prepare(const uint8_t* data, size_t len, PngJob& j)
{
    if (parse(data, len, j.h, false)) return j.rc = GAMUT_HIP_ERR_DECODE;
    if (!j.h.idata) return j.rc = set_error(GAMUT_HIP_ERR_DECODE, "png: no IDAT");
    const uint32_t bpl = (j.h.x * (uint32_t)j.h.depth + 7) / 8;                       // (stb's guess of the inflated size, stbdec.d:1809-1810: per component, not row_bytes())
    if (!inflate_idat(j.h.idata, j.h.ioff, (size_t)bpl * j.h.y * j.h.img_n + j.h.y, &j.raw_len, !j.h.is_iphone, j.raw)) return j.rc = GAMUT_HIP_ERR_DECODE;
    return j.rc = GAMUT_HIP_OK;
}

SlicePlan plan_slices(const std::vector<uint32_t>& idat_len, const std::vector<int64_t>& slot_bytes, const std::vector<int>& streams, const SliceOverrides& overrides)
{
    SlicePlan p;
    p.blob_off.assign(idat_len.size(), 0);
    p.who = streams;
    // longest streams first: a stream is one workgroup for its whole length, and workgroups start in the order of the list -- with
    // more streams than compute units the long ones must not be the ones that start last
    std::stable_sort(p.who.begin(), p.who.end(), [&](int a, int b) { return idat_len[(size_t)a] > idat_len[(size_t)b]; });
    const size_t n = p.who.size();
    uint32_t longest = 0; int64_t largest_out = 0; uint64_t data_bytes = 0;
    for (int i : p.who) {
        p.len.push_back(idat_len[(size_t)i]);
        longest = std::max(longest, idat_len[(size_t)i]); largest_out = std::max(largest_out, slot_bytes[(size_t)i]);
        data_bytes += up16(idat_len[(size_t)i]);
    }
    // 1 MiB slices; 512 KiB for up to 256 well-compressed large images, where a stream inflates more slowly than it arrives
    // (measured, 256 files: 4K of 12 MB 100 ms with 1 MiB slices, 127 with 512 KiB; 4K of 3.6 MB 60 / 57 ms; 1080p of 3.1 MB
    // 33 / 36 ms; 1024 files of 1080p 118 / 132 ms); at most 32 launches
    p.slice = (longest < (8u << 20) && n <= 256 && largest_out >= (16 << 20)) ? 1u << 19 : 1u << 20;
    if (overrides.slice) p.slice = overrides.slice;
    while ((uint64_t)p.slice * 32u < longest) p.slice *= 2;
    p.rounds = longest ? (int)(((uint64_t)longest + p.slice - 1) / p.slice) : 1;
    // The staging image.  One copy per (stream, slice) is a megabyte at a time: 37 GB/s on one copy stream where the link does 57
    // (tools/microbench/h2d_streams.hip, profiles/r04_h2d_streams.txt).  With every stream's share `pitch` bytes apart -- the
    // streams in the order of the list, longest first, so that those still running in a round are a prefix -- slice r of all of
    // them is ONE pitched copy (hipMemcpy2DAsync: 57 GB/s even with 512 KiB rows).  Batches of very unequal streams (the pitched
    // image would be more than twice the data) keep their tight layout and piece-wise copies, spread over two copy streams (46 GB/s).
    p.pitch = (uint64_t)p.rounds * p.slice;
    p.pitched = overrides.pitched >= 0 ? overrides.pitched != 0 : p.pitch * n <= 2 * data_bytes + (64u << 20);
    p.blob_bytes = p.pitched ? p.pitch * n : data_bytes;
    uint64_t at = 0;
    for (size_t k = 0; k < n; ++k) { p.blob_off[(size_t)p.who[k]] = p.pitched ? k * p.pitch : at; at += up16(p.len[k]); }
    // the units of work, slice-major: (round, stream); an empty stream has its one unit in round 0
    p.units_in_round.assign((size_t)p.rounds, 0);
    for (int r = 0; r < p.rounds; ++r)
        for (size_t k = 0; k < n; ++k)
            if ((uint64_t)r * p.slice < p.len[k] || (r == 0 && p.len[k] == 0)) { p.units.emplace_back(r, (int)k); ++p.units_in_round[(size_t)r]; }
    return p;
}

void copy_idat_range(const IdatSegments& segments, uint32_t skip, uint64_t lo, uint64_t hi, uint8_t* dst)
{
    uint64_t at = 0; const uint64_t want_lo = lo + skip, want_hi = hi + skip;
    for (const auto& sg : segments) {
        const uint64_t s_lo = at, s_hi = at + sg.second;
        at = s_hi;
        if (s_hi <= want_lo) continue;
        if (s_lo >= want_hi) break;
        const uint64_t c_lo = std::max(s_lo, want_lo), c_hi = std::min(s_hi, want_hi);
        memcpy(dst + (c_lo - want_lo), sg.first + (c_lo - s_lo), (size_t)(c_hi - c_lo));
    }
}

} // namespace gamut
