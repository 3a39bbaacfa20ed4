// bmp.hip -- BMP on the GPU: the pixels of stbi__bmp_load (source/gamut/codecs/stbdec.d:2263-2465) and the bytes of write_bmp
// (source/gamut/codecs/bmpenc.d:25-114), many images per launch.
//
// Decode.  The format has no serial chain: an output pixel is a function of 1 bit .. 4 bytes of its file.  The files of a batch go
// up in one blob through pinned staging, each placed so that its PIXEL DATA starts 16-byte aligned (rows are multiples of 4 bytes,
// so every row is then dword aligned); what lies behind the end of a file is zero in the blob and file positions >= its length are
// never loaded, which is the reference's reader handing out zeros (stbi__get8).  One launch decodes all images: an image record per
// file, and units of (image, row, segment of 256 lanes) found from the records' running unit counts, as the QOI encoder finds its
// tiles.  A lane takes 4 pixels (8 of a 1-bit file): up to 16 bytes in, up to 16 bytes (32 for 1-bit -> rgba) out, into the unit's
// run in LDS.  The palette of a unit's image sits in LDS as (R, G, B, 255) words, entries from the palette size on as (0, 0, 0, 255) -- DEVIATION: the reference reads uninitialised
// stack memory for such an index.  req_comp 1 / 2 (stbi__convert_format: stbi__compute_y) happen in the same store.
//
// The all_a rule (:2137, :2418, :2439-2443) is the one global dependency: a 32-bit BI_RGB file (header size other than 12) whose alpha
// bytes are ALL zero is given alpha 255 when the target has an alpha channel.  Each wave ORs the alpha bytes it decodes and, if the
// result is not zero, issues one atomicOr into the image's word; a second, small launch -- only when the batch holds such a file --
// rewrites the alpha of the images whose word stayed 0.
//
// Encode.  The 122-byte BITMAPV4 header is built on the host and copied by the kernel.  The pixel body behind it is ONE run of bytes
// (rows bottom-up, padded to 4 bytes) that starts at out_offset + 122, in general not even 4-aligned.  A workgroup makes 4096 bytes of
// it in LDS from aligned dword loads of the source (any pitch, any alignment; v_alignbyte_b32 / v_perm_b32) and stores them as aligned
// 16-byte chunks, head and tail by bytes.  Decode stores its units' bytes the same way (flush_run).  DEVIATION: the 0..3 pad bytes
// of a 24-bit row, which the reference writes from an uninitialised malloc buffer, are zero.
#include "encode_host.hpp"
#include "device_util.hpp"

namespace gamut {
int bmp_parse_header(const uint8_t* data, size_t len, int req_comp, gamut_hip_bmp_info* info);     // bmp_host.hip
namespace {

constexpr int kThreads = 256;
constexpr int kFileHeader = 122;                                             // 14 + DIB_SIZE 108 (bmpenc.d:33-37)

struct DecImg {
    const uint8_t* file;                                                     // device address of the file's byte 0
    int64_t  out_off;
    uint32_t avail;                                                          // file bytes in the blob; positions >= avail read as zero
    uint32_t pix_off, stride, w, h;
    uint32_t unit0, segs;                                                    // units [unit0, unit0 + h * segs) of the batch
    uint32_t pal_pos, pal_esz, psize;
    uint32_t mask[4];                                                        // r g b a
    int8_t   shift[4]; uint8_t bits[4], mul[4], down[4];                     // stbi__shiftsigned's operands per channel
    uint8_t  bpp, comps, target, top_down, easy, cand;                       // bpp: 1 4 8 16 24 32 as the reference reads the rows
    uint8_t  pad[2];
    uint32_t word;                                                           // the image's alpha-OR word
};

// stbi__shiftsigned(v & mask, shift, bits) :2493-2511
__device__ __forceinline__ uint32_t channel(const DecImg& im, uint32_t v, int c)
{
    uint32_t x = v & im.mask[c];
    const int s = im.shift[c];
    x = s < 0 ? x << -s : x >> s;
    x >>= 8 - im.bits[c];
    return (x * im.mul[c]) >> im.down[c];
}

__device__ __forceinline__ uint32_t luma(uint32_t px) { return ((px & 255u) * 77u + (px >> 8 & 255u) * 150u + (px >> 16 & 255u) * 29u) >> 8; }   // stbi__compute_y

__global__ __launch_bounds__(kThreads) void k_bmp_decode(const DecImg* imgs, int n_img, uint8_t* out, uint32_t* alpha_or)
{
    __shared__ uint32_t pal[256];
    __shared__ uint32_t run[kThreads * 8 + 4];                               // the unit's output bytes: 256 lanes x up to 32
    const uint32_t u = blockIdx.x;
    const DecImg im = imgs[find_unit<&DecImg::unit0>(imgs, n_img, u)];
    const uint32_t lu = u - im.unit0, j = lu / im.segs, seg = lu - j * im.segs;
    const uint32_t tid = threadIdx.x;
    if (im.bpp <= 8) {                                                       // (uniform over the workgroup)
        uint32_t e = 0xFF000000u;                                            // pal[i][3] = 255 :2338; (0, 0, 0) from psize on
        if (tid < im.psize) {
            const uint64_t p = (uint64_t)im.pal_pos + tid * im.pal_esz;      // B, G, R (, reserved) :2334-2337
            e |= file_byte(im, p + 2) | file_byte(im, p + 1) << 8 | file_byte(im, p) << 16;
        }
        pal[tid] = e;
        __syncthreads();
    }
    const uint32_t ppl = im.bpp == 1 ? 8u : 4u;                               // pixels per lane
    const uint32_t lane = seg * kThreads + tid;
    const uint64_t x0 = (uint64_t)lane * ppl;
    uint32_t a_or = 0;
    if (x0 < im.w) {
        const uint32_t cnt = min(ppl, im.w - (uint32_t)x0);
        const uint32_t nbytes = ppl * im.bpp / 8;                            // 1, 2, 4, 8, 12, 16
        const uint64_t rel = (uint64_t)j * im.stride + (uint64_t)lane * nbytes;           // from the first pixel byte
        uint32_t v[4] = { 0, 0, 0, 0 };
        if (nbytes >= 4) {
            #pragma unroll
            for (int k = 0; k < 4; ++k) if ((uint32_t)k * 4 < nbytes) v[k] = file_dword(im, im.pix_off + rel + 4 * k);
        } else {
            v[0] = file_dword(im, im.pix_off + (rel & ~(uint64_t)3)) >> (8 * (uint32_t)(rel & 3));
        }
        uint32_t px[8];
        #pragma unroll
        for (int i = 0; i < 8; ++i) {
            px[i] = 0;
            if ((uint32_t)i >= cnt) continue;
            uint32_t p;
            if (im.bpp == 1) p = pal[(v[0] >> (7 - i)) & 1u];                // MSB first :2348-2359
            else if (im.bpp == 4) { const uint32_t b = byte_of(v, (i & 3) >> 1); p = pal[(i & 1) ? (b & 15u) : (b >> 4)]; }   // high nibble first :2366-2376
            else if (im.bpp == 8) p = pal[byte_of(v, i & 3)];
            else if (im.bpp == 24) p = byte_of(v, 3 * (i & 3) + 2) | byte_of(v, 3 * (i & 3) + 1) << 8 | byte_of(v, 3 * (i & 3)) << 16 | 0xFF000000u;   // :2413-2417
            else {
                const uint32_t val = im.bpp == 16 ? (v[(i & 3) >> 1] >> (16 * (i & 1))) & 0xFFFFu : v[i & 3];
                if (im.easy) p = __builtin_amdgcn_perm(val, val, 0x03000102u);            // B G R A -> R G B A
                else p = (channel(im, val, 0) & 255u) | (channel(im, val, 1) & 255u) << 8 | (channel(im, val, 2) & 255u) << 16 |
                         (im.mask[3] ? (channel(im, val, 3) & 255u) : 255u) << 24;         // :2426-2431
            }
            px[i] = p;
            a_or |= p >> 24;
        }
        // the store: comps bytes per pixel; 1 / 2 through stbi__compute_y (stbi__convert_format), alpha only where the target has one
        uint32_t ob[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        #pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (im.comps == 4) ob[i] = px[i];
            else if (im.comps == 3) { set_byte(ob, 3 * i, px[i] & 255u); set_byte(ob, 3 * i + 1, px[i] >> 8 & 255u); set_byte(ob, 3 * i + 2, px[i] >> 16 & 255u); }
            else if (im.comps == 2) { set_byte(ob, 2 * i, luma(px[i])); set_byte(ob, 2 * i + 1, im.target == 4 ? px[i] >> 24 : 255u); }
            else set_byte(ob, i, luma(px[i]));
        }
        const uint32_t nb = cnt * im.comps, at = tid * ppl * im.comps / 4;     // <= 32 bytes, at a dword of the run
        #pragma unroll
        for (int k = 0; k < 8; ++k) if ((uint32_t)k * 4 < nb) run[at + k] = ob[k];
    }
    __syncthreads();
    {
        const uint64_t xs = (uint64_t)seg * kThreads * ppl;                  // the unit's first pixel; (uniform over the workgroup)
        const uint32_t y = im.top_down ? j : im.h - 1 - j;                   // the reference flips bottom-up files :2445-2454
        flush_run<kThreads>(run, out + im.out_off + ((uint64_t)y * im.w + xs) * im.comps, (uint32_t)min((uint64_t)kThreads * ppl, im.w - xs) * im.comps, tid);
    }
    if (im.cand) {                                                           // (uniform over the workgroup: every lane takes part)
        #pragma unroll
        for (int d = 32; d; d >>= 1) a_or |= __shfl_xor(a_or, d);
        if ((tid & 63u) == 0 && a_or) atomicOr(&alpha_or[im.word], a_or);
    }
}

// :2439-2443 for the images of `cand` whose alpha bytes were all zero: alpha 255 (the last byte of an rgba8 / la8 pixel)
__global__ __launch_bounds__(kThreads) void k_bmp_alpha(const DecImg* imgs, const int* cand, const uint32_t* alpha_or, uint8_t* out)
{
    const DecImg im = imgs[cand[blockIdx.y]];
    if (alpha_or[im.word] != 0) return;
    const uint64_t npx = (uint64_t)im.w * im.h;
    uint8_t* o = out + im.out_off + (im.comps - 1);
    for (uint64_t p = (uint64_t)blockIdx.x * kThreads + threadIdx.x; p < npx; p += (uint64_t)gridDim.x * kThreads) o[p * im.comps] = 255;
}

int high_bit(uint32_t z) { int n = -1; while (z) { ++n; z >>= 1; } return n; }            // stbi__high_bit :2468
int bitcount(uint32_t a) { int n = 0; while (a) { n += a & 1u; a >>= 1; } return n; }     // stbi__bitcount :2480

// Measurements (tools/bmp_bench.py): with GAMUT_HIP_BMP_TIMING=1 the decode call brackets its kernels -- not the upload -- with events
// and keeps the GPU time of the calling thread's last call; the blob is resident in HBM when the first event is reached.
thread_local float t_last_decode_kernel_ms = -1.0f;

int decode_batch(const uint8_t* const* data, const size_t* len, int count, int req_comp, const int64_t* out_offset, uint8_t* out,
                 gamut_hip_bmp_info* info, int* status_host, hipStream_t stream)
{
    static const uint8_t kMul[9] = { 0, 0xff, 0x55, 0x49, 0x11, 0x21, 0x41, 0x81, 0x01 }, kDown[9] = { 0, 0, 0, 1, 0, 2, 4, 6, 0 };   // :2495-2502
    std::vector<DecImg> imgs; std::vector<int> which, cand; std::vector<size_t> file0;
    int first_bad = -1, first_rc = GAMUT_HIP_OK; char first_msg[200] = { 0 };
    uint64_t units = 0; size_t cursor = 0; uint32_t words = 0;
    for (int i = 0; i < count; ++i) {
        gamut_hip_bmp_info bi;
        int rc = bmp_parse_header(data[i], len[i], req_comp, &bi);
        const int target = req_comp >= 3 ? req_comp : bi.channels_in_file;
        if (rc == GAMUT_HIP_OK && out_offset[i] < 0) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "bmp: negative out_offset");
        if (info) info[i] = bi;
        if (status_host) status_host[i] = rc;
        if (rc != GAMUT_HIP_OK) {
            if (first_bad < 0) { first_bad = i; first_rc = rc; snprintf(first_msg, sizeof(first_msg), "%s", last_error_buf()); }
            continue;
        }
        DecImg im{};
        im.out_off = out_offset[i];
        im.w = (uint32_t)bi.width; im.h = (uint32_t)bi.height;
        im.bpp = (uint8_t)(bi.bpp < 16 ? bi.bpp : bi.bpp == 16 ? 16 : bi.bpp == 24 ? 24 : 32);        // :2390-2392, :2424
        const uint64_t row_bytes = im.bpp == 1 ? ((uint64_t)im.w + 7) >> 3 : im.bpp == 4 ? ((uint64_t)im.w + 1) >> 1 : (uint64_t)im.w * (im.bpp / 8);
        im.stride = (uint32_t)((row_bytes + 3) & ~(uint64_t)3);
        im.pix_off = (uint32_t)bi.pixel_offset;
        const uint64_t need = (uint64_t)im.pix_off + (uint64_t)im.stride * im.h;
        im.avail = (uint32_t)std::min<uint64_t>(len[i], need);
        im.comps = (uint8_t)(req_comp ? req_comp : bi.channels_in_file); im.target = (uint8_t)target;
        im.top_down = (uint8_t)bi.top_down;
        im.psize = (uint32_t)bi.palette_size; im.pal_esz = bi.header_size == 12 ? 3 : 4;
        im.pal_pos = 14u + (uint32_t)bi.header_size + ((bi.header_size == 40 || bi.header_size == 56) && bi.compression == 3 ? 12u : 0u);
        const uint32_t m[4] = { bi.mask_r, bi.mask_g, bi.mask_b, bi.mask_a };
        for (int c = 0; c < 4; ++c) {
            const int bits = bitcount(m[c]);
            im.mask[c] = m[c]; im.shift[c] = (int8_t)(high_bit(m[c]) - 7); im.bits[c] = (uint8_t)bits;
            im.mul[c] = kMul[bits > 8 ? 0 : bits]; im.down[c] = kDown[bits > 8 ? 0 : bits];
        }
        im.easy = im.bpp == 32 && m[2] == 0xffu && m[1] == 0xff00u && m[0] == 0x00ff0000u && m[3] == 0xff000000u;             // :2396-2398
        im.cand = bi.header_size != 12 && bi.bpp == 32 && bi.compression == 0 && target == 4 && (im.comps == 4 || im.comps == 2);   // all_a starts at 0 :2137
        im.word = words;
        if (im.cand) { cand.push_back((int)imgs.size()); ++words; }
        const uint32_t per_unit = (im.bpp == 1 ? 8u : 4u) * kThreads;
        im.segs = (im.w + per_unit - 1) / per_unit;
        im.unit0 = (uint32_t)units;
        units += (uint64_t)im.h * im.segs;
        if (units > 0x7FFFFFFFull) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "bmp_decode: batch of more than 2^31 units");
        const size_t lead = (16 - ((cursor + im.pix_off) & 15)) & 15;       // the pixel data 16-byte aligned in the blob
        file0.push_back(cursor + lead);
        cursor = up16(cursor + lead + im.avail + 4) + 16;                    // zero bytes behind the file: a dword load that begins inside it ends inside the blob
        imgs.push_back(im); which.push_back(i);
    }
    if (!imgs.empty()) {
        const int n = (int)imgs.size();
        const size_t o_blob = 0, o_img = up256(cursor), o_word = o_img + up256(n * sizeof(DecImg)), o_cand = o_word + up256((size_t)words * 4 + 4),
                     total = o_cand + up256(cand.size() * 4 + 4);
        static thread_local PerDevice<DeviceScratch> scratch_pd;
        static thread_local PerDevice<PinnedScratch> pinned_pd;
        uint8_t* d = (uint8_t*)scratch_pd.cur().get(total, stream);
        uint8_t* h = pinned_pd.cur().get(total, stream);
        if (!d || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "bmp_decode: staging of %zu bytes failed", total);
        size_t prev_end = 0;
        for (int k = 0; k < n; ++k) {
            const size_t at = file0[(size_t)k], end = k + 1 < n ? file0[(size_t)k + 1] : cursor;
            memset(h + prev_end, 0, at - prev_end);
            memcpy(h + at, data[which[(size_t)k]], imgs[(size_t)k].avail);
            prev_end = at + imgs[(size_t)k].avail;
            if (k + 1 == n) memset(h + prev_end, 0, end - prev_end);
            imgs[(size_t)k].file = d + o_blob + at;
        }
        memcpy(h + o_img, imgs.data(), n * sizeof(DecImg));
        memset(h + o_word, 0, (size_t)words * 4 + 4);
        if (!cand.empty()) memcpy(h + o_cand, cand.data(), cand.size() * 4);
        GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, stream));
        const DecImg* dimg = (const DecImg*)(d + o_img);
        static const bool timing = env_flag("GAMUT_HIP_BMP_TIMING");
        KernelTimer<2> timer(timing);
        timer.mark(stream);
        hipLaunchKernelGGL(k_bmp_decode, dim3((uint32_t)units), dim3(kThreads), 0, stream, dimg, n, out, (uint32_t*)(d + o_word));
        for (size_t c0 = 0; c0 < cand.size(); c0 += 65535)                 // (grid.y holds 65535)
            hipLaunchKernelGGL(k_bmp_alpha, dim3(64, (uint32_t)std::min<size_t>(65535, cand.size() - c0)), dim3(kThreads), 0, stream, dimg,
                               (const int*)(d + o_cand) + c0, (const uint32_t*)(d + o_word), out);
        if (int rc = launch_status("bmp_decode")) return rc;
        timer.mark(stream);
        GAMUT_HIP_CHECK(hipStreamSynchronize(stream));
        timer.finish(&t_last_decode_kernel_ms);
    }
    if (first_bad >= 0) return set_error(first_rc, "image %d: %s", first_bad, first_msg);
    return GAMUT_HIP_OK;
}

// ---- encode -------------------------------------------------------------------------------------------------------------------
struct EncImg {
    const uint8_t* src; int64_t pitch; int64_t out_off;
    uint32_t w, h, comp, stride;
    uint32_t unit0, units;                                                   // units of kEncRun body bytes
    uint32_t hdr, pad;                                                       // index of the image's header in the header table
};

constexpr uint32_t kEncRun = 4096;                                           // body bytes per workgroup

// 4 source bytes at row offset k (a multiple of 4 from the row's first byte; may lie in front of the row or behind it): aligned
// dword loads of the words that hold at least one byte of the row, shifted together; bytes outside the row come out as anything
__device__ __forceinline__ uint32_t src_dword(const uint8_t* srow, uint32_t row_bytes, int k)
{
    if (k + 4 <= 0 || k >= (int)row_bytes) return 0u;
    const uint8_t* p = srow + k; const uint8_t* end = srow + row_bytes;
    const uint32_t m = (uint32_t)((uintptr_t)p & 3u);
    const uint8_t* q = p - m;
    const uint32_t lo = (q + 4 > srow && q < end) ? *reinterpret_cast<const uint32_t*>(q) : 0u;
    const uint32_t hi = (m && q + 8 > srow && q + 4 < end) ? *reinterpret_cast<const uint32_t*>(q + 4) : 0u;
    return __builtin_amdgcn_alignbyte(hi, lo, m);
}

// One workgroup writes kEncRun bytes of an image's pixel body.  Rows are multiples of 4 bytes, so a dword of the body lies in one
// row: a thread makes it from the source dwords around it (bgra: one byte permute; bgr: the 12-byte period of 4 pixels, three
// permutes by the dword's phase), pad bytes zero, into LDS; flush_run then stores the run at whatever alignment out_offset + 122 has.
__global__ __launch_bounds__(kThreads) void k_bmp_encode(const EncImg* imgs, int n_img, const uint8_t* headers, uint8_t* out)
{
    __shared__ uint32_t run[kEncRun / 4 + 4];
    const uint32_t u = blockIdx.x;
    const EncImg im = imgs[find_unit<&EncImg::unit0>(imgs, n_img, u)];
    const uint32_t lu = u - im.unit0, tid = threadIdx.x;
    uint8_t* file = out + im.out_off;
    if (lu == 0 && tid < (uint32_t)kFileHeader) file[tid] = headers[(size_t)im.hdr * 128 + tid];
    const uint64_t body_len = (uint64_t)im.stride * im.h, b0 = (uint64_t)lu * kEncRun;
    const uint32_t n = (uint32_t)min((uint64_t)kEncRun, body_len - b0), row_bytes = im.w * im.comp;
    for (uint32_t d = tid; d < n / 4; d += kThreads) {
        const uint64_t rb = b0 + 4ull * d;
        const uint32_t j = (uint32_t)(rb / im.stride), rr = (uint32_t)(rb - (uint64_t)j * im.stride);
        const uint8_t* srow = im.src + (int64_t)(im.h - 1 - j) * im.pitch;   // rows bottom-up (bmpenc.d:105)
        uint32_t v;
        if (im.comp == 4) {
            const uint32_t b = src_dword(srow, row_bytes, (int)rr);
            v = __builtin_amdgcn_perm(b, b, 0x03000102u);                    // R G B A -> B G R A
        } else {
            const uint32_t phase = (rr >> 2) % 3u;                           // which dword of the 12 bytes of 4 pixels
            const uint32_t b = src_dword(srow, row_bytes, (int)rr);
            const uint32_t a = phase ? src_dword(srow, row_bytes, (int)rr - 4) : 0u, c = phase < 2 ? src_dword(srow, row_bytes, (int)rr + 4) : 0u;
            if (phase == 0) v = __builtin_amdgcn_perm(c, b, 0x05000102u);                                           // b2 b1 b0 c1
            else if (phase == 1) v = (__builtin_amdgcn_perm(b, a, 0x07000304u) & 0xFF00FFFFu) | (c & 255u) << 16;   // b0 a3 c0 b3
            else v = __builtin_amdgcn_perm(b, a, 0x05060702u);                                                      // a2 b3 b2 b1
            const uint32_t valid = row_bytes - rr;                           // the 0..3 pad bytes of the row are zero
            if (valid < 4) v &= (1u << (8 * valid)) - 1u;
        }
        run[d] = v;
    }
    __syncthreads();
    flush_run<kThreads>(run, file + kFileHeader + b0, n, tid);
}

int64_t encode_bound(int w, int h, int comp)                                  // plugins/bmp.d:174-189
{
    if ((comp != 3 && comp != 4) || w < 1 || h < 1 || w > 32767 || h > 32767) return 0;
    return (int64_t)kFileHeader + (int64_t)h * ((w * comp + 3) & ~3);
}

void put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

void build_header(uint8_t* hdr, int w, int h, int comp, int ppm_x, int ppm_y)   // bmpenc.d:48-92
{
    memset(hdr, 0, 128);
    hdr[0] = 0x42; hdr[1] = 0x4d;
    put32(hdr + 2, (uint32_t)encode_bound(w, h, comp));
    put32(hdr + 10, kFileHeader);
    put32(hdr + 14, 108);
    put32(hdr + 18, (uint32_t)w); put32(hdr + 22, (uint32_t)h);
    hdr[26] = 1; hdr[28] = (uint8_t)(comp * 8);
    put32(hdr + 30, comp == 3 ? 0u : 3u);
    put32(hdr + 38, (uint32_t)ppm_x); put32(hdr + 42, (uint32_t)ppm_y);
    if (comp == 4) { hdr[56] = 0xff; hdr[59] = 0xff; hdr[62] = 0xff; hdr[69] = 0xff; }
    hdr[70] = 'B'; hdr[71] = 'G'; hdr[72] = 'R'; hdr[73] = 's';
}

int encode_batch(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width, const int32_t* height, const int32_t* comp,
                 const int32_t* ppm_x, const int32_t* ppm_y, int count, const int64_t* out_offset, uint8_t* out, int64_t* out_len,
                 int* status_host, hipStream_t stream)
{
    std::vector<EncImg> imgs; std::vector<int> which; std::vector<uint8_t> headers;
    struct Key { int w, h, c, px, py; }; std::vector<Key> keys;
    int first_bad = -1;
    uint64_t units = 0;
    for (int i = 0; i < count; ++i) {
        out_len[i] = 0;
        const int64_t bound = encode_bound(width[i], height[i], comp[i]);
        const bool ok = bound > 0 && src[i] && out_offset[i] >= 0;
        if (status_host) status_host[i] = ok ? GAMUT_HIP_OK : GAMUT_HIP_ERR_INVALID_ARG;
        if (!ok) { if (first_bad < 0) first_bad = i; continue; }
        EncImg im{};
        im.src = src[i]; im.pitch = src_pitch[i]; im.out_off = out_offset[i];
        im.w = (uint32_t)width[i]; im.h = (uint32_t)height[i]; im.comp = (uint32_t)comp[i]; im.stride = (im.w * im.comp + 3) & ~3u;
        const Key key{ width[i], height[i], comp[i], ppm_x ? ppm_x[i] : 0, ppm_y ? ppm_y[i] : 0 };
        size_t hi = 0;                                                       // one header per distinct (w, h, comp, ppm)
        for (; hi < keys.size(); ++hi) if (!memcmp(&keys[hi], &key, sizeof(Key))) break;
        if (hi == keys.size()) { keys.push_back(key); headers.resize(headers.size() + 128); build_header(headers.data() + hi * 128, key.w, key.h, key.c, key.px, key.py); }
        im.hdr = (uint32_t)hi;
        im.unit0 = (uint32_t)units; im.units = (uint32_t)(((uint64_t)im.stride * im.h + kEncRun - 1) / kEncRun);
        units += im.units;
        if (units > 0x7FFFFFFFull) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "bmp_encode: batch of more than 2^31 units");
        imgs.push_back(im); which.push_back(i);
    }
    if (!imgs.empty()) {
        const int n = (int)imgs.size();
        const size_t o_img = 0, o_hdr = up256(n * sizeof(EncImg)), total = o_hdr + up256(headers.size());
        static thread_local PerDevice<DeviceScratch> scratch_pd;
        static thread_local PerDevice<PinnedScratch> pinned_pd;
        uint8_t* d = (uint8_t*)scratch_pd.cur().get(total, stream);
        uint8_t* h = pinned_pd.cur().get(total, stream);
        if (!d || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "bmp_encode: scratch allocation of %zu bytes failed", total);
        memcpy(h + o_img, imgs.data(), n * sizeof(EncImg));
        memcpy(h + o_hdr, headers.data(), headers.size());
        GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, o_hdr + headers.size(), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_bmp_encode, dim3((uint32_t)units), dim3(kThreads), 0, stream, (const EncImg*)(d + o_img), n, (const uint8_t*)(d + o_hdr), out);
        if (int rc = launch_status("bmp_encode")) return rc;
        GAMUT_HIP_CHECK(hipStreamSynchronize(stream));
        for (int k = 0; k < n; ++k) { const int i = which[(size_t)k]; out_len[i] = encode_bound(width[i], height[i], comp[i]); }
    }
    if (first_bad >= 0) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "image %d: bmp_encode: refused shape or source", first_bad);
    return GAMUT_HIP_OK;
}

} // namespace
} // namespace gamut

using namespace gamut;

extern "C" {

int gamut_hip_bmp_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, int req_comp, const int64_t* out_offset,
                                      uint8_t* out, gamut_hip_bmp_info* info, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || req_comp < 0 || req_comp > 4 || (count > 0 && (!data || !len || !out_offset || !out)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "bmp_decode_batch_device: bad arguments (req_comp is 0..4)");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return decode_batch(data, len, count, req_comp, out_offset, out, info, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "bmp_decode_batch_device: out of host memory");
    }
}

float gamut_hip_bmp_last_decode_kernel_ms(void) { return t_last_decode_kernel_ms; }

int64_t gamut_hip_bmp_encode_bound(int width, int height, int comp) { return encode_bound(width, height, comp); }

int gamut_hip_bmp_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width, const int32_t* height,
                                      const int32_t* comp, const int32_t* ppm_x, const int32_t* ppm_y, int count, const int64_t* out_offset,
                                      uint8_t* out, int64_t* out_len, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!src || !src_pitch || !width || !height || !comp || !out_offset || !out || !out_len)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "bmp_encode_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return encode_batch(src, src_pitch, width, height, comp, ppm_x, ppm_y, count, out_offset, out, out_len, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "bmp_encode_batch_device: out of host memory");
    }
}

void* gamut_hip_bmp_write_to_mem(const void* data, int pitch, int w, int h, int comp, int ppm_x, int ppm_y, int* out_len)
{
    clear_error();
    if (!data || !out_len || encode_bound(w, h, comp) == 0 || encode_bound(w, h, comp) > 0x7fffffffLL) {     // (the length is handed back through an int)
        set_error(GAMUT_HIP_ERR_INVALID_ARG, "bmp_write_to_mem: invalid arguments"); return nullptr;
    }
    if (!have_device()) return nullptr;
    const int32_t W = w, H = h, Cc = comp, PX = ppm_x, PY = ppm_y;
    return encode_host_image("bmp_write_to_mem", HostRows{ data, pitch, (size_t)w * comp, h, 1, 0 }, (size_t)encode_bound(w, h, comp), out_len,
        [&](const uint8_t* src, int64_t spitch, int64_t, int64_t off, uint8_t* d, int64_t* n, hipStream_t st) {
            int status = 0;
            return encode_batch(&src, &spitch, &W, &H, &Cc, &PX, &PY, 1, &off, d, n, &status, st);
        });
}

} // extern "C"
