// gif_host.hip -- the GIF container on the host: GIFDecoder.open and the container part of decodeNextFrame (source/gamut/codecs/gif.d)
// restated, so that gamut_hip_gif_read_header gives the reference's verdict on a file without touching a GPU, and so that the batch
// decoder (gif.hip) gets, per frame, what its kernels need: rectangle, row order, palette, disposal and the LZW payload in one piece.
//
// The reader is io.d's memory stream (:386-452): a read fails when its bytes are not all there, a skip (seek) fails only when it would
// end PAST the end of the file.
//
// The reference walks the file twice and so does this: the counting pass of parseHeader (:152-184, needDecode == false: the LCT is
// skipped, no disposal, but every LZW code is walked, so its verdict includes the raster), then one parseFrame per layer.  What
// persists from the first pass into the second is kept: gce, `transparent` and the alpha bytes parseGraphicsControlExt pokes into the
// GCT -- a first frame without a GCE sees the LAST GCE of the file.  The second pass cannot fail where the first did not (it reads the
// same bytes), so the verdict of open is the verdict on the file.
//
// Two forms of the first pass:
//   * code walk (gamut_hip_gif_read_header): parseImageData :628-764 with needDecode == false, byte for byte on the sub-block chain;
//   * chain walk (the batch decoder): the sub-block chain is followed to its terminator and copied into one payload; the codes are
//     walked by k_gif_lzw, whose status word is the raster verdict.  The two agree because the reference leaves a frame's data either
//     at a terminator it read itself or, after an end code, by skipping the rest of the chain -- both end where the chain ends, and
//     a chain that runs into the end of the file is an error whichever way the codes turn out (a needed byte is missing, or the skip
//     behind the end code fails).
//
// The row order of a frame is the reference's stepping (stbi__out_gif_code :775-825) run row by row: a pixel at or below the screen's
// lower edge is dropped WITHOUT stepping on, so the rows that land are a prefix of the stream's rows; a frame lower than 8 rows paints
// rows outside itself (the lower edge is tested only after a row), and after pass 3 the walk goes on in steps of 2.  frameW == 0 acts
// as a width of 1.  The four passes visit disjoint rows, so a screen row has at most one stream row.
//
// DELIBERATE DEVIATIONS from the reference (in each it reads or writes memory it does not own):
//   * both palette buffers start zeroed (the reference's are uninitialised malloc memory): an index past every table ever read gives
//     an undrawn pixel;
//   * a frame with neither a local nor a global colour table (the reference dereferences null): refused;
//   * a frame with frameX + max(frameW, 1) > logicalScreenWidth (the reference wraps such rows into the next row and, on the last
//     row, writes past its heap block): refused.  A frame overhanging the BOTTOM is no deviation: its rows are dropped as in the reference;
//   * a screen of more than 2^29 - 1 pixels (the reference's int byte counts overflow): refused.
#include "gif_host.hpp"

namespace gamut {
namespace {

struct Reader {                                                    // io.d's MemoryFile
    const uint8_t* p; size_t len; size_t pos = 0;
    bool read(void* dst, size_t n) { if (len - pos < n) return false; memcpy(dst, p + pos, n); pos += n; return true; }
    int get8(bool& err) { if (pos >= len) { err = true; return 0; } err = false; return p[pos++]; }
    int get16(bool& err) { if (len - pos < 2) { pos = len; err = true; return 0; } err = false; pos += 2; return p[pos - 2] | p[pos - 1] << 8; }
    bool skip(size_t n) { if (n > len - pos) return false; pos += n; return true; }
};

struct Walker {
    Reader s;
    int W = 0, H = 0;
    bool has_gct = false;
    uint8_t gct[1024], lct[1024];
    int transparent = -1;
    int disposal = 0, transFlag = 0, delay = 0;                    // gce
    bool firstFrame = true;
    bool walk_codes = false;
    GifParsed* out = nullptr;                                      // second pass only
    size_t first_palette = 0;                                      // where this file's palettes begin in out->palettes

    int durationMs() const { return delay == 0 || delay == 1 ? 100 : delay * 10; }

    bool skipSubblocks()
    {
        int size; bool err;
        do { size = s.get8(err); if (err) return false; if (!s.skip((size_t)size)) return false; } while (size);
        return true;
    }
    bool graphicsControl()                                         // parseGraphicsControlExt :484-532
    {
        bool err;
        const int size = s.get8(err); if (err || size != 4) return false;
        const int rdit = s.get8(err); if (err) return false;
        disposal = (rdit >> 2) & 3; transFlag = rdit & 1;
        delay = s.get16(err); if (err) return false;
        const int index = s.get8(err); if (err) return false;
        if (transparent >= 0 && has_gct) gct[4 * transparent + 3] = 255;
        if (transFlag) { transparent = index; if (has_gct) gct[4 * transparent + 3] = 0; }
        else transparent = -1;
        const int zero = s.get8(err);
        return !err && zero == 0;
    }
    bool colortable(uint8_t* pal, int n, int transp)               // parseColortable :827-839
    {
        for (int i = 0; i < n; ++i) { if (!s.read(pal + 4 * i, 3)) return false; pal[4 * i + 3] = transp == i ? 0 : 255; }
        return true;
    }
    // parseImageData :628-764 with needDecode == false, the bytes taken from the sub-block chain as the reference takes them
    bool codeWalk(int lzw_cs)
    {
        bool err;
        const int clear = 1 << lzw_cs;
        int first = 1, codesize = lzw_cs + 1, codemask = (1 << codesize) - 1, bits = 0, valid_bits = 0;
        int avail = clear + 2, oldcode = -1, len = 0;
        for (;;) {
            if (valid_bits < codesize) {
                if (len == 0) { len = s.get8(err); if (err) return false; if (len == 0) return true; }
                --len;
                const int nb = s.get8(err); if (err) return false;
                bits |= nb << valid_bits; valid_bits += 8;
            } else {
                const int code = bits & codemask;
                bits >>= codesize; valid_bits -= codesize;
                if (code == clear) { codesize = lzw_cs + 1; codemask = (1 << codesize) - 1; avail = clear + 2; oldcode = -1; first = 0; }
                else if (code == clear + 1) {
                    if (!s.skip((size_t)len)) return false;
                    len = s.get8(err); if (err) return false;
                    while (len > 0) { if (!s.skip((size_t)len)) return false; len = s.get8(err); if (err) return false; }
                    return true;
                } else if (code <= avail) {
                    if (first) return false;
                    if (oldcode >= 0) { if (++avail > 8192) return false; }
                    else if (code == avail) return false;
                    if ((avail & codemask) == 0 && avail <= 0x0FFF) { codesize++; codemask = (1 << codesize) - 1; }
                    oldcode = code;
                } else return false;
            }
        }
    }
    // the chain alone; `dst`: where the data bytes go (second pass)
    bool chainWalk(std::vector<uint8_t>* dst)
    {
        bool err;
        for (;;) {
            const int size = s.get8(err); if (err) return false;
            if (size == 0) return true;
            if ((size_t)size > s.len - s.pos) return false;
            if (dst) dst->insert(dst->end(), s.p + s.pos, s.p + s.pos + size);
            s.pos += (size_t)size;
        }
    }
    bool lzwImage(bool needDecode, int dispose)                    // parseLWZImage :553-612
    {
        bool err;
        const int fx = s.get16(err); if (err) return false;
        const int fy = s.get16(err); if (err) return false;
        const int fw = s.get16(err); if (err) return false;
        const int fh = s.get16(err); if (err) return false;
        const int flags = s.get8(err); if (err) return false;
        const bool interlaced = (flags & 0x40) != 0;
        const uint8_t* pal = has_gct ? gct : nullptr;
        if (flags & 0x80) {
            const int lctSize = 1 << ((flags & 7) + 1);
            if (needDecode) { if (!colortable(lct, lctSize, transFlag ? transparent : -1)) return false; }
            else if (!s.skip((size_t)lctSize * 3)) return false;
            pal = lct;
        }
        if (!pal) return false;                                                             // DEVIATION
        const int fwe = fw > 1 ? fw : 1;
        if (fx + fwe > W) return false;                                                     // DEVIATION
        const int lzw_cs = s.get8(err); if (err) return false;
        if (lzw_cs > 12) return false;
        if (!needDecode) return walk_codes ? codeWalk(lzw_cs) : chainWalk(nullptr);
        GifFrame f{};
        f.fx = fx; f.fy = fy; f.fw = fwe; f.dispose = dispose; f.lzw_cs = lzw_cs; f.rowmap = -1;
        if (!interlaced) f.rows = fy < H ? H - fy : 0;
        else {
            static const int kStep[4] = { 8, 8, 4, 2 }, kStart[4] = { 0, 4, 2, 1 };
            f.rowmap = (int64_t)out->rowmaps.size();
            out->rowmaps.resize(out->rowmaps.size() + (size_t)H, (uint16_t)0xFFFF);
            uint16_t* map = out->rowmaps.data() + f.rowmap;
            int y = fy, pass = 0, r = 0;
            while (y < H) {
                map[y] = (uint16_t)r++;
                y += kStep[pass];
                if (y >= fy + fh && pass < 3) { ++pass; y = fy + kStart[pass]; }
            }
            f.rows = r;
        }
        if (out->palettes.size() == first_palette || memcmp(out->palettes.data() + out->palettes.size() - 256, pal, 1024) != 0) {
            out->palettes.resize(out->palettes.size() + 256);
            memcpy(out->palettes.data() + out->palettes.size() - 256, pal, 1024);
        }
        f.pal = (int32_t)(out->palettes.size() / 256 - 1);
        f.payload_off = out->payload.size();
        if (!chainWalk(&out->payload)) return false;
        f.payload_len = out->payload.size() - f.payload_off;
        out->frames.push_back(f);
        return true;
    }
    // parseFrame :346-462 -> 0 end of stream, 1 one frame, -1 error
    int parseFrame(bool needDecode)
    {
        int dispose = 0;
        if (firstFrame) firstFrame = false;
        else if (needDecode) dispose = disposal == 3 ? 2 : disposal;   // as the GCE stands when the frame starts; 3 is treated as 2 (:372-375)
        for (;;) {
            bool err;
            const int sep = s.get8(err); if (err) return -1;
            if (sep == 0x2C) return lzwImage(needDecode, dispose) ? 1 : -1;
            if (sep == 0x3B) return 0;
            if (sep != 0x21) return -1;
            const int label = s.get8(err); if (err) return -1;
            switch (label) {
            case 0x01: if (!s.skip(13) || !skipSubblocks()) return -1; break;
            case 0xF9: if (!graphicsControl()) return -1; break;
            case 0xFE: if (!skipSubblocks()) return -1; break;
            case 0xFF: { const int bs = s.get8(err); if (err || !s.skip((size_t)bs) || !skipSubblocks()) return -1; break; }
            default: return -1;
            }
        }
    }
};

} // namespace

int gif_fail(const char* why) { return set_error(GAMUT_HIP_ERR_DECODE, "gif: %s", why); }

int gif_parse(const uint8_t* data, size_t len, bool walk_codes, GifParsed* out, gamut_hip_gif_info* info)
{
    memset(info, 0, sizeof(*info));
    info->pixel_aspect_ratio = -1.0f;
    std::unique_ptr<Walker> wk(new Walker());
    Walker& w = *wk;
    w.s = Reader{ data, data ? len : 0 };
    w.walk_codes = walk_codes;
    memset(w.gct, 0, sizeof w.gct); memset(w.lct, 0, sizeof w.lct);                       // DEVIATION
    // ---- parseHeader :69-189
    char magic[6];
    if (!w.s.read(magic, 6)) return gif_fail("not a GIF");
    int is89;
    if (!memcmp(magic, "GIF87a", 6)) is89 = 0; else if (!memcmp(magic, "GIF89a", 6)) is89 = 1; else return gif_fail("not a GIF");
    bool err;
    w.W = w.s.get16(err); if (err) return gif_fail("short header");
    w.H = w.s.get16(err); if (err) return gif_fail("short header");
    const int flags = w.s.get8(err); if (err) return gif_fail("short header");
    w.s.get8(err); if (err) return gif_fail("short header");
    const int aspect = w.s.get8(err); if (err) return gif_fail("short header");
    if ((int64_t)w.W * w.H > 0x1FFFFFFFLL) return gif_fail("screen too large");           // DEVIATION
    if (flags & 0x80) {
        w.has_gct = true;
        if (!w.colortable(w.gct, 1 << ((flags & 7) + 1), -1)) return gif_fail("short global colour table");
    }
    const size_t offset = w.s.pos;
    int layers = 0; double sum = 0.0;
    for (;;) {
        const int res = w.parseFrame(false);
        if (res < 0) return gif_fail("damaged file");
        if (res == 0) break;
        ++layers; sum += w.durationMs();
    }
    info->width = w.W; info->height = w.H; info->layers = layers; info->is_gif89 = is89;
    info->pixel_aspect_ratio = aspect == 0 ? -1.0f : (aspect + 15.0f) / 64;
    info->fps = sum == 0 ? 10.0f : (float)(layers * 1000.0f / sum);
    if (!out) return GAMUT_HIP_OK;
    // ---- the second pass: one parseFrame per layer, with the state the first pass left behind
    w.s.pos = offset; w.firstFrame = true; w.out = out; w.first_palette = out->palettes.size();
    for (int l = 0; l < layers; ++l)
        if (w.parseFrame(true) != 1) return gif_fail("damaged file");
    return GAMUT_HIP_OK;
}

} // namespace gamut

using namespace gamut;

extern "C" int gamut_hip_gif_read_header(const uint8_t* data, size_t len, gamut_hip_gif_info* info)
{
    clear_error();
    if (!info) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "gif_read_header: info is NULL");
    try {
        return gif_parse(data, len, true, nullptr, info);
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "gif_read_header: out of host memory");
    }
}
