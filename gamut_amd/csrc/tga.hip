// tga.hip -- TGA on the GPU: the pixels of TGADecoder.decodeImage (source/gamut/codecs/tga.d:384-598), many files per call.
//
// The files of a batch go up in one blob through pinned staging, each at a 16-byte boundary, with zero bytes behind it; file
// positions >= the file's length are never loaded.  Two launches, whatever the batch holds:
//
// k_tga_unpacked -- types 1 / 2 / 3.  A unit is (image, file row, segment of 1024 pixels), found from the image records' running
// unit counts as bmp.hip finds its units.  The unit's source bytes (any alignment: the pixel data starts wherever the ID field and
// the colour map end) come into LDS through aligned dword loads and v_alignbyte_b32; a lane takes 4 pixels: the colour-map lookup
// (first 256 entries expanded once into LDS, an index >= palette_len reads entry 0), the 5-5-5 expansion (v * 255) / 31, the R/B
// swap, and the widening to req_comp 3 / 4 in one pass; the unit's output bytes are assembled in LDS and leave as aligned 16-byte
// stores with byte head and tail (flush_run, the discipline of bmp.hip).  The row flip is the store's address.  A file too short
// for its pixels or its colour map never gets here: the host refuses it by size arithmetic.
//
// k_tga_rle -- types 9 / 10 / 11.  The packets form a chain with no row index: next(p) = p + 1 + (cmd & 0x80 ? 1 : (cmd & 127) + 1)
// * bytes_per_source_pixel, and a packet may run across row ends.  One workgroup per file walks the stream in windows of kWin
// bytes counted from the first packet byte.  Per window: every byte position computes its own next (as if it were a command byte);
// the positions reachable from the window's entry offset are marked by pointer doubling (round r marks the chain members 2^r ..
// 2^(r+1) - 1 and squares the jump table; the loop ends as soon as the entry's jump leaves the window); a block scan over the marks
// gives each packet its number and, over the packets' pixel counts, its first output pixel; the lanes then expand pixels, each by a
// binary search over that prefix.  The window's exit offset (where the chain leaves it) and the pixel count carry to the next
// window.  kWin + 528 bytes are loaded, so a packet that starts on a window's last byte has its pixels in LDS.  The reference
// stops at width * height pixels, so the surplus of the last packet is dropped; every pixel checks that the bytes it reads lie in
// the file (the reference's read fails otherwise), and a stream that ends early -- at a command byte or inside pixel data --
// refuses the WHOLE file (status word, GAMUT_HIP_ERR_DECODE).  Bottom-up files are flipped at the store: pixel i goes to row
// h - 1 - i / w.
//
// Kept from the reference: the colour map starts palette_start BYTES behind the ID field; 15 / 16-bit entries and pixels are not
// R/B swapped; 16-bit grey is two raw bytes.  DEVIATION: width * height * components > 2^31 - 1 is refused (tga_host.hip).
#include "common.hpp"
#include "device_util.hpp"

namespace gamut {
int tga_parse_header(const uint8_t* data, size_t len, gamut_hip_tga_info* info);                   // tga_host.hip
int tga_fail(const char* why);
namespace {

constexpr int kThreads = 256;
constexpr int kSegPx = 4 * kThreads;                                         // pixels of an unpacked unit
constexpr int kPalLds = 256;                                                 // colour-map entries kept in LDS; the rest is read from the file
constexpr int kWin = 4096;                                                   // bytes of an RLE window
constexpr int kWinLoad = kWin + 528;                                         // + the longest packet (1 + 128 * 4) behind the last byte, dword multiple
constexpr int kPerLane = kWin / kThreads;                                    // window positions a lane owns in the scan

struct TgaImg {
    const uint8_t* file;                                                     // device address of the file's byte 0 (16-byte aligned)
    int64_t  out_off;
    uint32_t avail;                                                          // the file's length
    uint32_t pix_off, pal_off, pal_len;
    uint32_t w, h;
    uint32_t unit0, segs;                                                    // unpacked: units [unit0, unit0 + h * segs) of the batch
    uint32_t status;                                                         // RLE: index of the file's status word
    uint8_t  bps, comps, outc, indexed, rgb16, bottom_up, pal_esz, pad;      // bps: bytes per source pixel; comps: the file's; outc: stored
};

// n bytes of the file from position `from` (any alignment) into LDS dwords S[0 ..): aligned loads, v_alignbyte_b32
__device__ __forceinline__ void stage_bytes(const TgaImg& im, uint64_t from, uint32_t n, uint32_t* S, uint32_t tid)
{
    const uint64_t a = from & ~(uint64_t)3;
    const uint32_t sh = (uint32_t)(from & 3u);
    for (uint32_t d = tid; d < (n + 3) / 4; d += kThreads) {
        const uint32_t lo = file_dword(im, a + 4ull * d), hi = sh ? file_dword(im, a + 4ull * d + 4) : 0u;
        S[d] = __builtin_amdgcn_alignbyte(hi, lo, sh);
    }
}

// up to 4 little-endian source bytes -> the pixel in the file's own components, byte 0 first
//   rgb16: stbi__tga_read_rgb16 :625-646 (already R, G, B);  3 / 4 components: the R/B swap :577-587;  1 / 2: raw
__device__ __forceinline__ uint32_t conv(uint32_t raw, uint32_t comps, uint32_t rgb16)
{
    if (rgb16) {
        const uint32_t r = (raw >> 10) & 31u, g = (raw >> 5) & 31u, b = raw & 31u;
        return (r * 255u) / 31u | ((g * 255u) / 31u) << 8 | ((b * 255u) / 31u) << 16;
    }
    if (comps >= 3) return __builtin_amdgcn_perm(raw, raw, 0x03000102u);     // B G R A -> R G B A
    return raw;
}

__device__ __forceinline__ uint32_t pal_entry_from_file(const TgaImg& im, uint32_t idx)
{
    const uint64_t p = (uint64_t)im.pal_off + (uint64_t)idx * im.pal_esz;
    uint32_t raw = 0;
    for (uint32_t k = 0; k < im.pal_esz; ++k) raw |= file_byte(im, p + k) << (8 * k);
    return conv(raw, im.comps, im.rgb16);
}

__device__ __forceinline__ void load_palette(const TgaImg& im, uint32_t* pal, uint32_t tid)
{
    if (im.indexed && tid < (uint32_t)kPalLds && tid < im.pal_len) pal[tid] = pal_entry_from_file(im, tid);
}

// source pixel -> what is stored: outc bytes, byte 0 first.  req_comp 3 / 4 is convertTo(rgb8 / rgba8): grey replicated, a missing
// alpha 255, alpha dropped (by storing 3 bytes)
__device__ __forceinline__ uint32_t pixel(const TgaImg& im, const uint32_t* pal, uint32_t raw)
{
    uint32_t px;
    if (im.indexed) {
        uint32_t idx = im.bps == 1 ? raw & 255u : raw & 0xFFFFu;
        if (idx >= im.pal_len) idx = 0;                                      // :514-518
        px = idx < (uint32_t)kPalLds ? pal[idx] : pal_entry_from_file(im, idx);
    } else {
        px = conv(raw, im.comps, im.rgb16);
    }
    if (im.outc == im.comps) return px;
    if (im.comps == 1) return (px & 255u) * 0x010101u | 0xFF000000u;
    if (im.comps == 2) return (px & 255u) * 0x010101u | (px & 0xFF00u) << 16;
    if (im.comps == 3) return px | 0xFF000000u;
    return px;
}

__global__ __launch_bounds__(kThreads) void k_tga_unpacked(const TgaImg* imgs, int n_img, uint8_t* out)
{
    __shared__ uint32_t pal[kPalLds];
    __shared__ uint32_t src[kSegPx + 4];                                     // the unit's source bytes: 1024 pixels x up to 4
    __shared__ uint32_t run[kSegPx + 8];                                     // the unit's output bytes
    const uint32_t u = blockIdx.x, tid = threadIdx.x;
    const TgaImg im = imgs[find_unit<&TgaImg::unit0>(imgs, n_img, u)];
    const uint32_t lu = u - im.unit0, j = lu / im.segs, seg = lu - j * im.segs;
    const uint32_t x0 = seg * kSegPx, npx = min((uint32_t)kSegPx, im.w - x0);   // (uniform over the workgroup)
    load_palette(im, pal, tid);
    stage_bytes(im, (uint64_t)im.pix_off + ((uint64_t)j * im.w + x0) * im.bps, npx * im.bps, src, tid);
    __syncthreads();
    uint8_t* runb = reinterpret_cast<uint8_t*>(run);
    #pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t x = tid * 4 + i;
        if (x >= npx) break;
        uint32_t raw = 0;
        for (uint32_t k = 0; k < im.bps; ++k) raw |= byte_of(src, x * im.bps + k) << (8 * k);
        const uint32_t px = pixel(im, pal, raw);
        if (im.outc == 4) run[x] = px;
        else for (uint32_t k = 0; k < im.outc; ++k) runb[x * im.outc + k] = (uint8_t)(px >> (8 * k));
    }
    __syncthreads();
    const uint32_t y = im.bottom_up ? im.h - 1 - j : j;                      // :426 / :557-572
    flush_run<kThreads>(run, out + im.out_off + ((uint64_t)y * im.w + x0) * im.outc, npx * im.outc, tid);
}

__device__ __forceinline__ uint32_t packet_pixels(uint32_t cmd) { return (cmd & 127u) + 1u; }
__device__ __forceinline__ uint32_t packet_next(uint32_t j, uint32_t cmd, uint32_t bps) { return j + 1u + ((cmd & 0x80u) ? 1u : packet_pixels(cmd)) * bps; }

__global__ __launch_bounds__(kThreads) void k_tga_rle(const TgaImg* imgs, uint8_t* out, uint32_t* status)
{
    __shared__ uint32_t pal[kPalLds];
    __shared__ uint32_t win32[kWinLoad / 4];
    __shared__ uint16_t nxt[2][kWin + 2];                                    // the jump table, double buffered; [kWin] is the way out
    __shared__ uint8_t  mark[kWin];
    __shared__ uint16_t ppos[kWin / 2];                                      // packet -> window position (a packet has 2 bytes at least)
    __shared__ uint32_t ppix[kWin / 2 + 1];                                  // packet -> first pixel of the window's output
    __shared__ uint32_t sc[kThreads];
    __shared__ uint32_t bad;
    const uint32_t tid = threadIdx.x;
    const TgaImg im = imgs[blockIdx.x];
    const uint8_t* win = reinterpret_cast<const uint8_t*>(win32);
    const uint32_t npix = im.w * im.h, bps = im.bps;
    load_palette(im, pal, tid);
    if (tid == 0) bad = 0;
    uint64_t wstart = im.pix_off;                                            // file position of the window's byte 0
    uint32_t entry = 0, done = 0;                                            // (uniform over the workgroup, as everything the loop branches on)
    while (true) {
        __syncthreads();                                                     // the last window's readers are through
        stage_bytes(im, wstart, kWinLoad, win32, tid);
        __syncthreads();
        for (uint32_t j = tid; j < (uint32_t)kWin; j += kThreads) {
            nxt[0][j] = (uint16_t)min(packet_next(j, win[j], bps), (uint32_t)kWin);
            mark[j] = j == entry;
        }
        if (tid == 0) { nxt[0][kWin] = kWin; nxt[1][kWin] = kWin; }
        __syncthreads();
        // pointer doubling: before round r the table is next^(2^r) and the chain members 0 .. 2^r - 1 are marked
        int cur = 0;
        for (int r = 0; r < 12; ++r) {
            if (nxt[cur][entry] >= kWin) break;                              // everything between the entry and the way out is marked
            for (uint32_t j = tid; j < (uint32_t)kWin; j += kThreads) {
                const uint32_t t = nxt[cur][j];
                if (mark[j] && t < (uint32_t)kWin) mark[t] = 1;              // (a mark seen early marks a chain member too)
                nxt[cur ^ 1][j] = nxt[cur][t];
            }
            __syncthreads();
            cur ^= 1;
        }
        // packets and pixels in front of each lane's kPerLane positions: one scan over (pixels << 12 | packets)
        uint32_t mine = 0;
        #pragma unroll
        for (uint32_t i = 0; i < (uint32_t)kPerLane; ++i) { const uint32_t j = tid * kPerLane + i; if (mark[j]) mine += packet_pixels(win[j]) << 12 | 1u; }
        sc[tid] = mine;
        __syncthreads();
        for (uint32_t off = 1; off < (uint32_t)kThreads; off <<= 1) {
            const uint32_t t = tid >= off ? sc[tid - off] : 0u;
            __syncthreads();
            sc[tid] += t;
            __syncthreads();
        }
        const uint32_t total = sc[kThreads - 1], npk = total & 0xFFFu, wpix = total >> 12;
        {
            uint32_t k = (sc[tid] - mine) & 0xFFFu, p = (sc[tid] - mine) >> 12;
            #pragma unroll
            for (uint32_t i = 0; i < (uint32_t)kPerLane; ++i) {
                const uint32_t j = tid * kPerLane + i;
                if (mark[j]) { ppos[k] = (uint16_t)j; ppix[k] = p; ++k; p += packet_pixels(win[j]); }
            }
            if (tid == 0) ppix[npk] = wpix;
        }
        __syncthreads();
        const uint32_t take = min(wpix, npix - done);                        // the reference stops at width * height :473
        for (uint32_t p = tid; p < take; p += kThreads) {
            uint32_t lo = 0, hi = npk - 1;
            while (lo < hi) { const uint32_t mid = (lo + hi + 1) >> 1; if (ppix[mid] <= p) lo = mid; else hi = mid - 1; }
            const uint32_t j = ppos[lo], cmd = win[j];
            const uint32_t s = j + 1u + ((cmd & 0x80u) ? 0u : (p - ppix[lo]) * bps);
            if (wstart + s + bps > im.avail) { bad = 1; continue; }          // the reference's read fails: command byte or pixel bytes missing
            uint32_t raw = 0;
            for (uint32_t k = 0; k < bps; ++k) raw |= (uint32_t)win[s + k] << (8 * k);
            const uint32_t px = pixel(im, pal, raw);
            const uint32_t i = done + p, row = i / im.w, col = i - row * im.w;
            const uint32_t y = im.bottom_up ? im.h - 1 - row : row;
            uint8_t* d = out + im.out_off + ((uint64_t)y * im.w + col) * im.outc;
            if (im.outc == 4 && ((uintptr_t)d & 3u) == 0) *reinterpret_cast<uint32_t*>(d) = px;
            else for (uint32_t k = 0; k < im.outc; ++k) d[k] = (uint8_t)(px >> (8 * k));
        }
        __syncthreads();
        done += take;
        if (bad) { if (tid == 0) status[im.status] = 1u; return; }
        if (done >= npix) return;
        const uint32_t last = ppos[npk - 1];
        entry = packet_next(last, win[last], bps) - (uint32_t)kWin;          // where the chain left the window
        wstart += (uint32_t)kWin;
    }
}

// Measurements (tools/tga_bench.py): with GAMUT_HIP_TGA_TIMING=1 the decode call brackets its kernels -- not the upload -- with events
// and keeps the GPU time of the calling thread's last call; the blob is resident in HBM when the first event is reached.
thread_local float t_last_decode_kernel_ms = -1.0f;

int decode_batch(const uint8_t* const* data, const size_t* len, int count, int req_comp, const int64_t* out_offset, uint8_t* out,
                 gamut_hip_tga_info* info, int* status_host, hipStream_t stream)
{
    std::vector<TgaImg> flat, rle; std::vector<int> which_flat, which_rle; std::vector<size_t> at_flat, at_rle;
    int first_bad = -1, first_rc = GAMUT_HIP_OK; char first_msg[200] = { 0 };
    uint64_t units = 0; size_t cursor = 0;
    auto refuse = [&](int i, int rc) {
        if (status_host) status_host[i] = rc;
        if (first_bad < 0 || i < first_bad) { first_bad = i; first_rc = rc; snprintf(first_msg, sizeof(first_msg), "%s", last_error_buf()); }
    };
    for (int i = 0; i < count; ++i) {
        gamut_hip_tga_info ti;
        int rc = tga_parse_header(data[i], len[i], &ti);
        if (info) info[i] = ti;
        if (status_host) status_host[i] = GAMUT_HIP_OK;
        if (rc == GAMUT_HIP_OK && out_offset[i] < 0) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "tga: negative out_offset");
        if (rc == GAMUT_HIP_OK && len[i] > 0x7fffffffu) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "tga: file of more than 2^31 - 1 bytes");
        TgaImg im{};
        if (rc == GAMUT_HIP_OK) {
            im.out_off = out_offset[i];
            im.avail = (uint32_t)len[i];
            im.w = (uint32_t)ti.width; im.h = (uint32_t)ti.height;
            im.comps = (uint8_t)ti.channels_in_file; im.outc = (uint8_t)(req_comp ? req_comp : ti.channels_in_file);
            im.indexed = (uint8_t)ti.indexed; im.rgb16 = (uint8_t)ti.rgb16; im.bottom_up = (uint8_t)ti.bottom_up;
            im.bps = (uint8_t)(ti.indexed ? ti.bpp / 8 : ti.rgb16 ? 2 : ti.channels_in_file);
            if ((uint64_t)im.w * im.h * im.outc > 0x7fffffffull) rc = tga_fail("too large");                              // DEVIATION
        }
        if (rc == GAMUT_HIP_OK) {
            uint64_t pos = (uint64_t)ti.data_offset;
            if (ti.indexed) {                                               // :439-465: skip palette_start BYTES, then the whole colour map
                im.pal_esz = (uint8_t)(ti.rgb16 ? 2 : ti.channels_in_file);
                im.pal_len = (uint32_t)ti.palette_len;
                pos += (uint32_t)ti.palette_start;
                im.pal_off = (uint32_t)pos;
                if (pos > len[i] || (uint64_t)im.pal_len * im.pal_esz > len[i] - pos) rc = tga_fail("file ends inside the colour map");
                pos += (uint64_t)im.pal_len * im.pal_esz;
            }
            im.pix_off = (uint32_t)pos;
            if (rc == GAMUT_HIP_OK && !ti.rle && (pos > len[i] || (uint64_t)im.w * im.h * im.bps > len[i] - pos)) rc = tga_fail("file ends inside the pixels");
        }
        if (rc != GAMUT_HIP_OK) { refuse(i, rc); continue; }
        const size_t at = cursor;                                            // the file's byte 0 at a 16-byte boundary, zeros behind it
        cursor = up16(cursor + im.avail + 8) + 16;
        if (ti.rle) {
            im.status = (uint32_t)rle.size();
            rle.push_back(im); which_rle.push_back(i); at_rle.push_back(at);
        } else {
            im.segs = (im.w + kSegPx - 1) / kSegPx;
            im.unit0 = (uint32_t)units;
            units += (uint64_t)im.h * im.segs;
            if (units > 0x7FFFFFFFull) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "tga_decode: batch of more than 2^31 units");
            flat.push_back(im); which_flat.push_back(i); at_flat.push_back(at);
        }
    }
    if (!flat.empty() || !rle.empty()) {
        const size_t nf = flat.size(), nr = rle.size();
        const size_t o_flat = up256(cursor), o_rle = o_flat + up256(nf * sizeof(TgaImg) + 4), o_st = o_rle + up256(nr * sizeof(TgaImg) + 4),
                     total = o_st + up256(nr * 4 + 4);
        static thread_local PerDevice<DeviceScratch> scratch_pd;
        static thread_local PerDevice<PinnedScratch> pinned_pd;
        uint8_t* d = (uint8_t*)scratch_pd.cur().get(total, stream);
        uint8_t* h = pinned_pd.cur().get(total, stream);
        if (!d || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "tga_decode: staging of %zu bytes failed", total);
        auto place = [&](TgaImg& im, size_t at, const uint8_t* bytes) {     // the file, and zeros up to the next file's place
            memcpy(h + at, bytes, im.avail);
            memset(h + at + im.avail, 0, up16(at + im.avail + 8) + 16 - (at + im.avail));
            im.file = d + at;
        };
        for (size_t k = 0; k < nf; ++k) place(flat[k], at_flat[k], data[which_flat[k]]);
        for (size_t k = 0; k < nr; ++k) place(rle[k], at_rle[k], data[which_rle[k]]);
        memset(h + cursor, 0, o_flat - cursor);
        memset(h + o_flat, 0, total - o_flat);
        if (nf) memcpy(h + o_flat, flat.data(), nf * sizeof(TgaImg));
        if (nr) memcpy(h + o_rle, rle.data(), nr * sizeof(TgaImg));
        GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, stream));
        static const bool timing = env_flag("GAMUT_HIP_TGA_TIMING");
        KernelTimer<2> timer(timing);
        timer.mark(stream);
        if (nf) hipLaunchKernelGGL(k_tga_unpacked, dim3((uint32_t)units), dim3(kThreads), 0, stream, (const TgaImg*)(d + o_flat), (int)nf, out);
        if (nr) hipLaunchKernelGGL(k_tga_rle, dim3((uint32_t)nr), dim3(kThreads), 0, stream, (const TgaImg*)(d + o_rle), out, (uint32_t*)(d + o_st));
        if (int rc = launch_status("tga_decode")) return rc;
        timer.mark(stream);
        if (nr) GAMUT_HIP_CHECK(hipMemcpyAsync(h + o_st, d + o_st, nr * 4, hipMemcpyDeviceToHost, stream));
        GAMUT_HIP_CHECK(hipStreamSynchronize(stream));
        timer.finish(&t_last_decode_kernel_ms);
        const uint32_t* st = (const uint32_t*)(h + o_st);
        for (size_t k = 0; k < nr; ++k)
            if (st[k]) { tga_fail("run-length stream ends before width * height pixels"); refuse(which_rle[k], GAMUT_HIP_ERR_DECODE); }
    }
    if (first_bad >= 0) return set_error(first_rc, "image %d: %s", first_bad, first_msg);
    return GAMUT_HIP_OK;
}

} // namespace
} // namespace gamut

using namespace gamut;

extern "C" {

int gamut_hip_tga_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, int req_comp, const int64_t* out_offset,
                                      uint8_t* out, gamut_hip_tga_info* info, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (req_comp != 0 && req_comp != 3 && req_comp != 4) || (count > 0 && (!data || !len || !out_offset || !out)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "tga_decode_batch_device: bad arguments (req_comp is 0, 3 or 4)");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return decode_batch(data, len, count, req_comp, out_offset, out, info, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "tga_decode_batch_device: out of host memory");
    }
}

int gamut_hip_tga_rle_window(void) { return kWin; }

float gamut_hip_tga_last_decode_kernel_ms(void) { return t_last_decode_kernel_ms; }

} // extern "C"
