// qoix.hip -- QOIX colour files on the GPU: the 8-bit rgb / rgba slice of qoix_lz4_decode (source/gamut/plugins/qoix.d:350-473), that is
// the LZ4 block of LZ4_decompress_fast (source/gamut/codecs/lz4.d:760-978) and the QOI2AVG op stream of qoix_decode
// (source/gamut/codecs/qoi2avg.d:624-897), many files per call.  The header is read on the host (qoix_host.hip).
//
// The files of a batch go up in one blob through pinned staging, each at a 16-byte boundary with zero bytes behind it; positions
// >= the file's length are never loaded.  Two launches, whatever a batch of colour files holds (grey files, behind
// gamut_hip_qoix_set_plane, add a third: k_qoix_plane, described where it stands):
//
// k_qoix_lz4 -- a wave per compressed file.  The sequence walk (token, length extensions, offset) is wave-uniform and reads its
// bytes from a 512-byte window of the file that the lanes hold a dword each (v_readlane); literal runs and matches are copied by
// the 64 lanes, 64 bytes a step.  A match's net effect in the reference is out[k] = out[k - offset] byte by byte (the 8-byte wild
// copies and the dec32table / dec64table step for offsets below 8 produce exactly that): a match with offset < 64 reads
// out[start + k mod offset], whose sources all lie in front of the match, so its steps do not depend on each other; a match with
// offset >= 64 may read what the previous step wrote, which relies on one wave's global accesses being served in issue order
// (gif.hip's string copy relies on the same rule: LLVM AMDGPUUsage, "Memory Model", gfx90a and later; the loop carries the
// compiler-level fence).  Every loop consumes input bytes or produces output bytes, every load is guarded by the file's length and
// every store by orig.  The inflated stream goes to a scratch slot sized from the file's orig claim.
//
// k_qoix_avg -- a wave per op stream.  The chain left pixel -> LOCO-I prediction -> next pixel is serial by construction, so the
// batch is the parallelism (as in k_gif_lzw) and the chain itself is kept wave-uniform (scalar values handed between the lanes'
// copies by v_readfirstlane); the lanes do what is wide: the stream is fetched 256 bytes ahead (a dword per lane, handed out by
// v_readlane), the 64-entry FIFO is one register across the lanes, runs are filled 64 pixels a step, and finished rows leave in
// whole aligned 16-byte pieces (flush_run; 3-channel rows are packed 256 pixels at a time first).  ONE row of rgba in LDS serves as
// current and previous row at once: slot x holds the pixel above until the current pixel replaces it, and the up-left pixel is
// carried in a register.  kRowCap pixels of LDS per wave (8 KiB, + 0.8 KiB of packing space: 17 waves' worth in a CU's 160 KiB, so
// 4 waves per SIMD are resident at 1080p); a wider row lives in a global scratch row instead, read and written the same way.
// A hostile stream cannot make the kernel spin: an ADIFF chain ends at `size`, the pixel loop at width * height.
//
// DELIBERATE DEVIATIONS.  In each of these the reference touches memory it does not own; every one is GAMUT_HIP_ERR_DECODE.
//   1. LZ4: any read at or past the end of the file refuses the file (the reference has no input bound).
//   2. LZ4: offset 0, or a match that starts before the first output byte, refuses the file (the reference reads up to 64 KiB in
//      front of its buffer).
//   3. QOI2AVG: an END opcode that is executed -- at p < chunks_len or through an ADIFF chain -- refuses the file (the reference
//      leaves the rest of the row as whatever its scanline buffer held; in rows 0 and 1 that is uninitialised malloc memory).
//   4. QOI2AVG: an op byte read at index >= size refuses the file (an ADIFF chain running through the last four bytes).
#include "common.hpp"
#include "device_util.hpp"

extern "C" int gamut_valid_load_flags(int flags);                              // image_host.hip

namespace gamut {
int qoix_parse_header(const uint8_t* data, size_t len, gamut_hip_qoix_info* info, uint32_t* sub_size);       // qoix_host.hip
int qoix_fail(const char* why);
bool qoix_plane_on();
namespace {

constexpr int kWave = 64;
constexpr uint32_t kRowCap = 2048;                                             // pixels of a row kept in LDS
constexpr uint32_t kStagePx = 4 * kWave;                                       // pixels of a 3-channel row packed at a time
constexpr uint32_t kHeader = 25;

struct QxLz {                                                                  // a compressed file
    const uint8_t* file;                                                       // device address of its byte 0 (16-byte aligned)
    uint8_t* dst;                                                              // where byte 0 of the inflated stream goes
    uint32_t avail, orig, status, pad;                                         // status: index of the file's status word
};
struct QxImg {                                                                 // an op stream
    const uint8_t* file;                                                       // byte 0 of what the sub-codec sees: the file itself, or its scratch slot
    uint32_t* wide_row;                                                        // w + 8 dwords of global scratch when w > kRowCap
    int64_t  out_off;
    uint32_t avail, w, h, status;                                              // avail: qoix_decode's `size`
    uint32_t outc, plane;                                                      // plane: a QOI-Plane stream (k_qoix_plane), else QOI2AVG
};

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ void wave_order() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }   // (compiler order only: one wave's LDS and global accesses are served in issue order)

// 512 bytes of a file around a wave-uniform read position, a dword per lane and chunk of 256; the next chunk is requested while
// the current one is used
template <class Rec> struct ByteWindow {
    uint32_t cur, nxt, idx;
    __device__ __forceinline__ void load(const Rec& r, uint32_t chunk, uint32_t lane)
    {
        idx = chunk;
        cur = file_dword(r, 256ull * chunk + 4u * lane);
        nxt = file_dword(r, 256ull * chunk + 256u + 4u * lane);
    }
    __device__ __forceinline__ void seek(const Rec& r, uint32_t c, uint32_t lane)                       // c: uniform, the chunk `cur` is to hold
    {
        if (c != idx) {
            if (c == idx + 1) { cur = nxt; idx = c; nxt = file_dword(r, 256ull * c + 256u + 4u * lane); }
            else load(r, c, lane);
        }
    }
    __device__ __forceinline__ uint32_t byte(const Rec& r, uint32_t pos, uint32_t lane)                 // pos: uniform
    {
        seek(r, pos >> 8, lane);
        return ((uint32_t)__builtin_amdgcn_readlane((int)cur, (int)((pos >> 2) & 63u)) >> (8u * (pos & 3u))) & 255u;
    }
    // dword d (0..127, its own per lane) of the 512 bytes held: one ds_bpermute from each half
    __device__ __forceinline__ uint32_t dword(uint32_t d) const
    {
        const uint32_t a = __shfl(cur, (int)(d & 63u)), b = __shfl(nxt, (int)(d & 63u));
        return d < 64u ? a : b;
    }
};

__global__ void __launch_bounds__(kWave) k_qoix_lz4(const QxLz* __restrict__ files, uint32_t* status)
{
    const QxLz f = files[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    const uint32_t iend = f.avail;
    const int64_t oend = f.orig;
    uint8_t* out = f.dst;
    ByteWindow<QxLz> win; win.load(f, 0, lane);
    uint32_t ip = kHeader + 4;
    int64_t op = 0;
    bool bad = false;
    while (true) {
        wave_order();
        // lz4.d:806-825 the token and the literal length
        if (ip >= iend) { bad = true; break; }                                 // DEVIATION 1
        const uint32_t token = win.byte(f, ip++, lane);
        uint64_t len = token >> 4;
        if (len == 15) {
            uint32_t s;
            do {
                if (ip >= iend) { bad = true; break; }                         // DEVIATION 1
                s = win.byte(f, ip++, lane);
                len += s;
            } while (s == 255);
            if (bad) break;
        }
        // :827-857 the literals
        if (len > (uint64_t)(iend - ip)) { bad = true; break; }                // DEVIATION 1: the literals are not all there
        const int64_t cpy = op + (int64_t)len;
        const bool last = cpy > oend - 8;
        if (last && cpy != oend) { bad = true; break; }                        // :842-845 must stop exactly there
        for (uint64_t k = lane; k < len; k += kWave) out[op + (int64_t)k] = file_byte(f, (uint64_t)ip + k);
        ip += (uint32_t)len; op = cpy;
        if (last) break;                                                       // whatever input follows is ignored
        // :859-882 offset and match length
        if (iend - ip < 2) { bad = true; break; }                              // DEVIATION 1
        const uint32_t offset = win.byte(f, ip, lane) | win.byte(f, ip + 1, lane) << 8;
        ip += 2;
        if (offset == 0 || (int64_t)offset > op) { bad = true; break; }        // DEVIATION 2
        uint64_t ml = token & 15u;
        if (ml == 15) {
            uint32_t s;
            do {
                if (ip >= iend) { bad = true; break; }                         // DEVIATION 1
                s = win.byte(f, ip++, lane);
                ml += s;
            } while (s == 255);
            if (bad) break;
        }
        ml += 4;
        if (op + (int64_t)ml > oend - 5) { bad = true; break; }                // :935-940 the last 5 bytes must be literals
        // :921-951 the match: out[op + k] = out[op + k - offset]
        const int64_t start = op - (int64_t)offset;
        if (offset < (uint32_t)kWave) {
            for (uint64_t k = lane; k < ml; k += kWave) out[op + (int64_t)k] = out[start + (int64_t)(k % offset)];
        } else {
            for (uint64_t k0 = 0; k0 < ml; k0 += kWave) {
                wave_order();                                                  // this step may read what the previous one wrote
                const uint64_t k = k0 + lane;
                if (k < ml) out[op + (int64_t)k] = out[start + (int64_t)k];
            }
        }
        op += (int64_t)ml;
    }
    if (bad && lane == 0) atomicOr(&status[f.status], 1u);
}

// LOCO-I per channel from left a, up b, up-left c (qoi2avg.d:843-897): c >= max gives min, c <= min gives max (max wins a tie),
// else a + b - c, which cannot leave 0..255 in that branch
__device__ __forceinline__ uint32_t loco1(uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t mx = max(a, b), mn = min(a, b);
    uint32_t p = a + b - c;
    if (c >= mx) p = mn;
    if (c <= mn) p = mx;
    return p & 255u;
}
__device__ __forceinline__ uint32_t loco_rgb(uint32_t a, uint32_t b, uint32_t c)
{
    return loco1(a & 255u, b & 255u, c & 255u) | loco1((a >> 8) & 255u, (b >> 8) & 255u, (c >> 8) & 255u) << 8 |
           loco1((a >> 16) & 255u, (b >> 16) & 255u, (c >> 16) & 255u) << 16;
}

// a finished row (rgba dwords, 4 readable dwords behind it) -> w * outc bytes at dst, any alignment
__device__ __forceinline__ void flush_row(const uint32_t* row, uint32_t* stage, uint8_t* dst, uint32_t w, uint32_t outc, uint32_t lane)
{
    wave_order();
    if (outc == 4) { flush_run<kWave>(row, dst, w * 4u, lane); wave_order(); return; }
    for (uint32_t x0 = 0; x0 < w; x0 += kStagePx) {                            // alpha dropped: 4 pixels -> 3 dwords per lane
        const uint32_t n = min(kStagePx, w - x0), q = 4u * lane;
        if (q < n) {
            const uint32_t a = row[x0 + q] & 0xFFFFFFu, b = q + 1 < n ? row[x0 + q + 1] & 0xFFFFFFu : 0u,
                           c = q + 2 < n ? row[x0 + q + 2] & 0xFFFFFFu : 0u, d = q + 3 < n ? row[x0 + q + 3] & 0xFFFFFFu : 0u;
            stage[3 * lane] = a | b << 24; stage[3 * lane + 1] = b >> 8 | c << 16; stage[3 * lane + 2] = c >> 16 | d << 8;
        }
        wave_order();
        flush_run<kWave>(stage, dst + 3ull * x0, n * 3u, lane);
        wave_order();
    }
}

// qoix_decode qoi2avg.d:697-836.  `row`: LDS (kWide false) or the file's global scratch row; slot x holds the pixel above (x, y)
// until pixel (x, y) is stored there.
template <bool kWide> __device__ __forceinline__ bool avg_decode(const QxImg& im, uint32_t* row, uint32_t* stage, uint8_t* out, uint32_t lane)
{
    const uint32_t w = im.w, h = im.h, size = im.avail, chunks_len = size - 4u, outc = im.outc;
    uint8_t* dst = out + im.out_off;
    ByteWindow<QxImg> win; win.load(im, 0, lane);
    uint32_t p = kHeader, px = 0xFF000000u, ul = 0, fifo = 0, fifo_pos = 0, x = 0, y = 0;
    // n pixels of px from (x, y) on, across row ends, cut at the image's end.  up: the old row[x] when the caller has read it (y > 0)
    auto put = [&](uint32_t n, uint32_t up, bool have_up) {
        while (n && y < h) {
            const uint32_t m = min(n, w - x);
            if (y > 0) ul = (m == 1 && have_up) ? up : rfl(row[x + m - 1]);      // the pixel above the last one stored: up-left of the next
            have_up = false;
            wave_order();
            if (m == 1) { if (lane == 0) row[x] = px; }
            else for (uint32_t k = lane; k < m; k += kWave) row[x + k] = px;
            x += m; n -= m;
            if (x == w) {
                flush_row(row, stage, dst + (uint64_t)y * w * outc, w, outc, lane);
                x = 0; ++y;
            }
        }
    };
    while (y < h) {
        if (p >= chunks_len) { put(0xFFFFFFFFu, 0, false); break; }            // :709 the stream is over: px repeats, no error
        uint32_t ref = px, up = 0;
        if (y > 0) {                                                           // :713-730
            up = rfl(row[x]);
            ref = x == 0 ? (up & 0xFFFFFFu) : loco_rgb(px, up, ul);            // (the reference pixel's alpha is never used)
        }
        uint32_t b1 = win.byte(im, p++, lane);
        while (b1 >= 0xe8u && b1 < 0xf0u) {                                    // ADIFF :768-771: the next op without re-testing p < chunks_len
            px = (px & 0xFFFFFFu) | ((px >> 24) + (b1 & 7u) - 4u) << 24;
            if (p >= size) return false;                                       // DEVIATION 4
            b1 = win.byte(im, p++, lane);
        }
        const uint32_t nbytes = b1 < 0xc0u ? 0u : b1 < 0xe0u ? 1u : b1 < 0xe8u ? 2u : b1 < 0xf8u ? 0u : b1 < 0xfdu ? 1u : b1 == 0xfdu ? 3u : b1 == 0xfeu ? 4u : 0u;
        if (nbytes > size - p) return false;                                   // DEVIATION 4 (p <= size here)
        uint32_t o[4] = { 0, 0, 0, 0 };
        #pragma unroll
        for (uint32_t k = 0; k < 4; ++k) if (k < nbytes) o[k] = win.byte(im, p++, lane);
        const uint32_t rr = ref & 255u, rg = (ref >> 8) & 255u, rb = (ref >> 16) & 255u, pa = px & 0xFF000000u;
        uint32_t run = 0; bool writes = true;
        if (b1 < 0x80u) {                                                      // LUMA :735-747
            const uint32_t vg = ((b1 >> 4) & 7u) - 4u, bias = (int32_t)vg < 0 ? 1u : 2u;
            px = ((rr + vg - bias + ((b1 >> 2) & 3u)) & 255u) | ((rg + vg) & 255u) << 8 | ((rb + vg - bias + (b1 & 3u)) & 255u) << 16 | pa;
        } else if (b1 < 0xc0u) {                                               // INDEX :748-750
            px = (uint32_t)__builtin_amdgcn_readlane((int)fifo, (int)(b1 & 63u)); writes = false;
        } else if (b1 < 0xe0u) {                                               // LUMA2 :751-758
            const uint32_t vg = (b1 & 31u) - 16u;
            px = ((rr + vg - 8u + (o[0] >> 4)) & 255u) | ((rg + vg) & 255u) << 8 | ((rb + vg - 8u + (o[0] & 15u)) & 255u) << 16 | pa;
        } else if (b1 < 0xe8u) {                                               // LUMA3 :759-767
            const uint32_t dv = b1 << 16 | o[0] << 8 | o[1], vg = ((dv >> 12) & 127u) - 64u;
            px = ((rr + vg + ((dv >> 6) & 63u) - 32u) & 255u) | ((rg + vg) & 255u) << 8 | ((rb + vg + (dv & 63u) - 32u) & 255u) << 16 | pa;
        } else if (b1 < 0xf8u) {                                               // RUN :772-774
            run = b1 & 7u; writes = false;
        } else if (b1 < 0xfcu) {                                               // RUN2 :775-777
            run = (b1 & 3u) << 8 | o[0]; writes = false;
        } else if (b1 == 0xfcu) {                                              // GRAY :778-784
            px = o[0] * 0x010101u | pa;
        } else if (b1 == 0xfdu) {                                              // RGB :785-790
            px = o[0] | o[1] << 8 | o[2] << 16 | pa;
        } else if (b1 == 0xfeu) {                                              // RGBA :791-797
            px = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
        } else return false;                                                   // END :798-800, DEVIATION 3
        if (writes) { if (lane == (fifo_pos & 63u)) fifo = px; ++fifo_pos; }
        put(1u + run, up, true);
    }
    return true;
}

__global__ void __launch_bounds__(kWave) k_qoix_avg(const QxImg* __restrict__ imgs, uint8_t* out, uint32_t* status)
{
    __shared__ uint32_t row[kRowCap + 8];
    __shared__ uint32_t stage[3 * kWave + 8];
    const QxImg im = imgs[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    if (status[im.status]) return;                                             // the LZ4 block was refused
    const bool ok = im.w > kRowCap ? avg_decode<true>(im, im.wide_row, stage, out, lane) : avg_decode<false>(im, row, stage, out, lane);
    if (!ok && lane == 0) atomicOr(&status[im.status], 2u);
}

// ---- QOI-Plane: qoiplane_decode (source/gamut/codecs/qoiplane.d:377-541), 8-bit luminance or luminance + alpha, behind
// gamut_hip_qoix_set_plane.  Ops sit on nibble boundaries; with first nibble n0 (and the one behind it, n1):
//   0..7 DIFF1 (1 nibble)   8,9 DIFF2 (2)   a DIRECT (3)   b n1>0 ADIFF (2)   b 0 LA (6)   c..e REPEAT1 (1)   f REPEAT2 (3)
// Neither an op's length nor its pixel count (ADIFF 0, REPEAT1 1 + (n0 & 3), REPEAT2 byte + 4 or "to the end" for byte 255, else 1)
// depends on a pixel value, so a wave takes the stream 64 nibbles at a time and the lanes parse:
//   * every lane holds the nibble at np + lane and the 5 behind it (ByteWindow fetches 256 bytes ahead; two ds_bpermute pairs);
//   * op starts: lane i's nibble maps "the next op starts o nibbles on" (o = 0..5) to o - 1, or to length - 1 for o = 0; the six
//     results are six bytes, composing two such maps is two v_perm_b32, and a 6-step scan over the lanes gives every lane the offset
//     it is entered with.  A group begins at an op start (np moves by 64 + the offset the last lane leaves), so the entry offset
//     carried between groups is always 0 and the scan is the pointer-doubling over the ops;
//   * pixel index: a prefix sum of the counts, saturating at the pixels still missing; an op at or past that point is surplus;
//   * alpha changes at LA (absolute) and by the LAST ADIFF in front of a pixel op (previous pixel's alpha + d - 8): a segmented
//     prefix sum over the lanes, (set, value) pairs;
//   * luminance: DIRECT / LA absolute, REPEAT the left pixel, DIFF (top + left + 1) / 2 + d.  Only this is a chain: a wave-uniform
//     loop over the group's pixel ops on scalar values.  `top` was fetched by the lanes before the loop (the row buffer holds the
//     pixel above until the pixel below replaces it); when the row is narrower than the group's pixels, top was produced inside
//     this group and is looked up among the lanes' results (a ballot and a v_readlane);
//   * the pixels go to ONE row in the OUTPUT's layout (1 or 2 bytes a pixel: `top` is channel 0 of the pixel above, as in the
//     reference, which reads it from its output) -- kPlaneCap pixels of LDS, 8 KiB a wave as k_qoix_avg, or a global scratch row --
//     single pixels by their lanes, runs 64 pixels a step; a finished row leaves through flush_run.
// Every group consumes at least one nibble, the walk ends at width * height.
// DEVIATION P1: an op of which a nibble lies at byte index >= size refuses the file (the reference has no input bound; the four closing
// bytes ARE decoded: f ff is "repeat to the end", which is how a stream ends).
constexpr uint32_t kPlaneCap = 4096;
enum : uint32_t { kPDiff = 0, kPAbs = 1, kPRep = 2, kPAdiff = 3 };

template <bool kWide> __device__ __forceinline__ bool plane_decode(const QxImg& im, uint32_t* row, uint8_t* out, uint32_t lane)
{
    const uint32_t w = im.w, outc = im.outc, total = w * im.h;                 // (< 400000000)
    const uint64_t nib_end = 2ull * im.avail;
    uint8_t* dst = out + im.out_off;
    uint8_t* rowb = reinterpret_cast<uint8_t*>(row);
    auto store = [&](uint32_t pos, uint32_t v) {
        if (outc == 1) rowb[pos] = (uint8_t)v; else reinterpret_cast<uint16_t*>(rowb)[pos] = (uint16_t)v;
    };
    ByteWindow<QxImg> win; win.load(im, 0, lane);
    uint64_t np = 2ull * kHeader;                                              // nibble index of the group's first op
    uint32_t done = 0, x = 0, y = 0, l = 0, a = 255, pend = 0;                 // pend: 0x100 | d of an ADIFF that ended the previous group
    while (done < total) {
        if (np >= nib_end) return false;                                       // DEVIATION P1
        wave_order();
        // the nibbles np + lane .. np + lane + 5
        const uint64_t q = np + lane;
        const uint32_t bp = (uint32_t)(q >> 1);
        win.seek(im, (uint32_t)(np >> 9), lane);
        const uint32_t dw = (bp >> 2) - 64u * win.idx;                         // 0..72
        const uint32_t raw = __builtin_amdgcn_alignbyte(win.dword(dw + 1), win.dword(dw), bp & 3u);      // bytes bp .. bp + 3
        const uint32_t nb = __builtin_bswap32(raw) << (4u * ((uint32_t)q & 1u));
        const uint32_t n0 = nb >> 28, n1 = (nb >> 24) & 15u, n2 = (nb >> 20) & 15u, n3 = (nb >> 16) & 15u, n45 = (nb >> 8) & 255u;
        const uint32_t len = n0 < 8u ? 1u : n0 < 10u ? 2u : n0 == 10u ? 3u : n0 == 11u ? (n1 ? 2u : 6u) : n0 == 15u ? 3u : 1u;
        // op starts
        uint32_t tlo = 0x02010000u | (len - 1u), thi = 0x00000403u;
        #pragma unroll
        for (uint32_t d = 1; d < kWave; d <<= 1) {
            const uint32_t olo = __shfl_up(tlo, d), ohi = __shfl_up(thi, d);
            if (lane >= d) {
                const uint32_t nlo = __builtin_amdgcn_perm(thi, tlo, olo), nhi = __builtin_amdgcn_perm(thi, tlo, ohi);
                tlo = nlo; thi = nhi;
            }
        }
        const uint32_t entered = __shfl_up(tlo, 1u) & 255u;
        const bool start = lane == 0 || entered == 0;
        const uint32_t leaves = (uint32_t)__builtin_amdgcn_readlane((int)tlo, 63) & 255u;
        // what the op does
        const uint32_t rem = total - done;
        uint32_t type, val = 0, cnt = 1;
        if (n0 < 8u) { type = kPDiff; val = n0 - 4u; }
        else if (n0 < 10u) { type = kPDiff; val = ((n0 & 1u) << 4 | n1) - 16u; }
        else if (n0 == 10u) { type = kPAbs; val = n1 << 4 | n2; }
        else if (n0 == 11u) { if (n1) { type = kPAdiff; cnt = 0; } else { type = kPAbs; val = n2 << 4 | n3; } }
        else if (n0 < 15u) { type = kPRep; cnt = 1u + (n0 & 3u); }
        else { type = kPRep; const uint32_t b = n1 << 4 | n2; cnt = b == 255u ? rem : b + 4u; }
        const bool is_la = n0 == 11u && n1 == 0;
        cnt = start ? min(cnt, rem) : 0u;
        uint32_t sum = cnt;                                                    // inclusive, saturating at rem
        #pragma unroll
        for (uint32_t d = 1; d < kWave; d <<= 1) {
            const uint32_t o = __shfl_up(sum, d);
            if (lane >= d) sum = min(sum + o, rem);
        }
        const uint32_t before = __shfl_up(sum, 1u);
        const uint32_t pix = lane ? before : 0u;                               // pixels of this group in front of the op
        const uint32_t group = (uint32_t)__builtin_amdgcn_readlane((int)sum, 63);
        const bool live = start && pix < rem;                                  // else surplus: never read
        if (__ballot(live && ((q + len - 1u) >> 1) >= im.avail)) return false; // DEVIATION P1
        cnt = min(cnt, rem - min(pix, rem));
        const bool pixop = live && type != kPAdiff;
        // alpha: (set << 8 | value) pairs; the last ADIFF in front of a pixel op adds d - 8 to the previous pixel's alpha
        const uint64_t lives = __ballot(live), below = lives & ((1ull << lane) - 1ull);
        const uint32_t adw = type == kPAdiff ? 0x100u | n1 : 0u;
        const uint32_t prev = __shfl(adw, below ? 63 - __builtin_clzll(below) : 0);
        const uint32_t front = below ? prev : pend;
        uint32_t av = 0;
        if (pixop) av = is_la ? 0x100u | n45 : (front & 0x100u) ? ((front & 15u) - 8u) & 255u : 0u;
        #pragma unroll
        for (uint32_t d = 1; d < kWave; d <<= 1) {
            const uint32_t o = __shfl_up(av, d);
            if (lane >= d && !(av & 0x100u)) av = (o & 0x100u) | ((o + av) & 255u);
        }
        const uint32_t ares = (av & 0x100u) ? av & 255u : (a + av) & 255u;
        a = (uint32_t)__builtin_amdgcn_readlane((int)ares, 63);
        pend = (uint32_t)__builtin_amdgcn_readlane((int)adw, 63 - __builtin_clzll(lives));               // (lane 0 is live)
        // top, where it was produced before this group: the pixel's index in the image is done + pix
        const uint32_t topkind = done + pix < w ? 0u : pix < w ? 1u : 2u;      // the left pixel (row 0) / fetched here / made in this group
        uint32_t topv = 0;
        if (pixop && type == kPDiff && topkind == 1u) { const uint32_t xi = x + pix; topv = rowb[(xi >= w ? xi - w : xi) * outc]; }
        // the chain, one straight-line step for every kind of op: l = ((top + left + 1) >> 1) + d, where an absolute op has top = left
        // = 0 and d = its value, and a REPEAT has top = left and d = 0 ((2 l + 1) >> 1 = l).  bit 8: left is the previous luminance
        // (else 0); bit 9: top is that same value (row 0, REPEAT); bit 10: top was made in this group
        const bool diff = type == kPDiff;
        const uint32_t opw = (val & 255u) | (type != kPAbs ? 0x100u : 0u) | (type == kPRep || (diff && topkind == 0u) ? 0x200u : 0u) |
                             (diff && topkind == 2u ? 0x400u : 0u);
        const uint64_t pixops = __ballot(pixop);
        uint32_t lres = 0;
        for (uint64_t m = pixops; m; m &= m - 1ull) {
            const int j = __builtin_ctzll(m);
            const uint32_t ow = (uint32_t)__builtin_amdgcn_readlane((int)opw, j);
            uint32_t top = (uint32_t)__builtin_amdgcn_readlane((int)topv, j);
            const uint32_t left = (ow & 0x100u) ? l : 0u;
            if (ow & 0x400u) {                                                 // the pixel op of this group that covers pixel pix - w
                const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)pix, j) - w;
                top = (uint32_t)__builtin_amdgcn_readlane((int)lres, 63 - __builtin_clzll(__ballot(pixop && pix <= t)));
            }
            top = (ow & 0x200u) ? left : top;
            l = (((top + left + 1u) >> 1) + ow) & 255u;
            lres = lane == (uint32_t)j ? l : lres;
        }
        // the pixels, row piece by row piece
        const uint32_t pv = lres | ares << 8;
        uint64_t runs = __ballot(pixop && cnt > 1u);
        for (uint32_t gp = 0; gp < group; ) {
            const uint32_t m = min(group - gp, w - x);
            wave_order();
            if (pixop && cnt == 1u && pix - gp < m) store(x + pix - gp, pv);
            for (uint64_t rm = runs; rm; rm &= rm - 1ull) {
                const int j = __builtin_ctzll(rm);
                const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)pix, j), e = s + (uint32_t)__builtin_amdgcn_readlane((int)cnt, j),
                               v = (uint32_t)__builtin_amdgcn_readlane((int)pv, j);
                if (s >= gp + m) break;
                if (e <= gp + m) runs &= ~(1ull << j);                         // ends in this piece
                for (uint32_t k = max(s, gp) + lane; k < min(e, gp + m); k += kWave) store(x + k - gp, v);
            }
            x += m; gp += m;
            if (x == w) {
                wave_order();
                flush_run<kWave>(row, dst + (uint64_t)y * w * outc, w * outc, lane);
                x = 0; ++y;
            }
        }
        done += group;
        np += 64u + leaves;
    }
    return true;
}

__global__ void __launch_bounds__(kWave) k_qoix_plane(const QxImg* __restrict__ imgs, uint8_t* out, uint32_t* status)
{
    __shared__ uint32_t row[kPlaneCap / 2 + 8];
    const QxImg im = imgs[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    if (status[im.status]) return;                                             // the LZ4 block was refused
    const bool ok = im.w > kPlaneCap ? plane_decode<true>(im, im.wide_row, out, lane) : plane_decode<false>(im, row, out, lane);
    if (!ok && lane == 0) atomicOr(&status[im.status], 2u);
}

// Measurements (tools/qoix_bench.py, tools/qoix_plane_bench.py): with GAMUT_HIP_QOIX_TIMING=1 the decode call brackets each of its
// kernels -- not the upload -- with events and keeps the GPU times of the calling thread's last call; the blob is resident in HBM when
// the first event is reached.
thread_local float t_last_ms[3] = { -1.0f, -1.0f, -1.0f };

int decode_batch(const uint8_t* const* data, const size_t* len, int count, int channels, const int64_t* out_offset, uint8_t* out,
                 gamut_hip_qoix_info* info, int* status_host, hipStream_t stream)
{
    std::vector<QxImg> imgs; std::vector<QxLz> lzs; std::vector<int> which; std::vector<size_t> at, slot, wide;
    int first_bad = -1, first_rc = GAMUT_HIP_OK; char first_msg[200] = { 0 };
    size_t cursor = 0, scratch = 0;
    auto refuse = [&](int i, int rc) {
        if (status_host) status_host[i] = rc;
        if (first_bad < 0 || i < first_bad) { first_bad = i; first_rc = rc; snprintf(first_msg, sizeof(first_msg), "%s", last_error_buf()); }
    };
    for (int i = 0; i < count; ++i) {
        gamut_hip_qoix_info qi; uint32_t size = 0;
        int rc = qoix_parse_header(data[i], len[i], &qi, &size);
        if (info) info[i] = qi;
        if (status_host) status_host[i] = GAMUT_HIP_OK;
        if (rc == GAMUT_HIP_OK && out_offset[i] < 0) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "qoix: negative out_offset");
        const bool plane = qi.channels < 3;                                    // (only with the switch on does such a header pass)
        if (rc == GAMUT_HIP_OK && channels && (channels < 3) != plane)
            rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "qoix: %d channels asked of a %d-channel file (1 / 2 are for grey files, 3 / 4 for colour files)", channels, qi.channels);
        if (rc != GAMUT_HIP_OK) { refuse(i, rc); continue; }
        QxImg im{};
        im.plane = plane;
        im.out_off = out_offset[i]; im.avail = size; im.w = (uint32_t)qi.width; im.h = (uint32_t)qi.height;
        im.outc = (uint32_t)(channels ? channels : qi.channels);
        im.status = (uint32_t)imgs.size();
        at.push_back(cursor);                                                  // the file's byte 0 at a 16-byte boundary, zeros behind it
        cursor = up16(cursor + len[i] + 8) + 16;
        size_t s = (size_t)-1, wr = (size_t)-1;
        if (qi.compression == 1) { s = scratch; scratch += up16((size_t)size + 8) + 16; }      // header-sized gap + orig bytes, read by whole dwords
        if (plane) { if (im.w > kPlaneCap) { wr = scratch; scratch += up16((size_t)im.w * 2 + 48); } }
        else if (im.w > kRowCap) { wr = scratch; scratch += up16(((size_t)im.w + 8) * 4); }
        slot.push_back(s); wide.push_back(wr);
        imgs.push_back(im); which.push_back(i);
    }
    if (!imgs.empty()) {
        const size_t n = imgs.size();
        size_t nlz = 0;
        for (size_t k = 0; k < n; ++k) nlz += slot[k] != (size_t)-1;
        const size_t o_img = up256(cursor), o_lz = o_img + up256(n * sizeof(QxImg)), o_st = o_lz + up256(nlz * sizeof(QxLz) + 4),
                     staged = o_st + up256(n * 4), total = staged + scratch;
        static thread_local PerDevice<DeviceScratch> scratch_pd;
        static thread_local PerDevice<PinnedScratch> pinned_pd;
        uint8_t* d = (uint8_t*)scratch_pd.cur().get(total, stream);
        uint8_t* h = pinned_pd.cur().get(staged, stream);
        if (!d || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "qoix_decode: staging of %zu bytes failed", total);
        lzs.reserve(nlz);
        for (size_t k = 0; k < n; ++k) {
            const size_t a = at[k], l = len[which[k]];
            memcpy(h + a, data[which[k]], l);
            memset(h + a + l, 0, up16(a + l + 8) + 16 - (a + l));
            imgs[k].file = d + a;
            if (slot[k] != (size_t)-1) {
                QxLz z{};
                z.file = d + a; z.dst = d + staged + slot[k] + kHeader; z.avail = (uint32_t)l; z.orig = imgs[k].avail - kHeader; z.status = imgs[k].status;
                lzs.push_back(z);
                imgs[k].file = d + staged + slot[k];
            }
            if (wide[k] != (size_t)-1) imgs[k].wide_row = (uint32_t*)(d + staged + wide[k]);
        }
        memset(h + cursor, 0, staged - cursor);
        size_t ncol = 0;                                                       // the colour records first, then the plane records
        for (size_t k = 0; k < n; ++k) ncol += !imgs[k].plane;
        for (size_t k = 0, c = 0, p = ncol; k < n; ++k) memcpy(h + o_img + (imgs[k].plane ? p++ : c++) * sizeof(QxImg), &imgs[k], sizeof(QxImg));
        if (nlz) memcpy(h + o_lz, lzs.data(), nlz * sizeof(QxLz));
        GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, staged, hipMemcpyHostToDevice, stream));
        static const bool timing = env_flag("GAMUT_HIP_QOIX_TIMING");
        KernelTimer<4> timer(timing);
        timer.mark(stream);
        if (nlz) hipLaunchKernelGGL(k_qoix_lz4, dim3((uint32_t)nlz), dim3(kWave), 0, stream, (const QxLz*)(d + o_lz), (uint32_t*)(d + o_st));
        timer.mark(stream);
        if (ncol) hipLaunchKernelGGL(k_qoix_avg, dim3((uint32_t)ncol), dim3(kWave), 0, stream, (const QxImg*)(d + o_img), out, (uint32_t*)(d + o_st));
        if (int rc = launch_status("qoix_decode")) return rc;
        timer.mark(stream);
        if (n > ncol) {                                                        // a third launch only when the batch holds a plane file
            hipLaunchKernelGGL(k_qoix_plane, dim3((uint32_t)(n - ncol)), dim3(kWave), 0, stream, (const QxImg*)(d + o_img) + ncol, out, (uint32_t*)(d + o_st));
            if (int rc = launch_status("qoix_decode (plane)")) return rc;
        }
        timer.mark(stream);
        GAMUT_HIP_CHECK(hipMemcpyAsync(h + o_st, d + o_st, n * 4, hipMemcpyDeviceToHost, stream));
        GAMUT_HIP_CHECK(hipStreamSynchronize(stream));
        timer.finish(t_last_ms);
        const uint32_t* st = (const uint32_t*)(h + o_st);
        for (size_t k = 0; k < n; ++k)
            if (st[k]) { qoix_fail(st[k] & 1u ? "the LZ4 block is damaged" : "the op stream is damaged"); refuse(which[k], GAMUT_HIP_ERR_DECODE); }
    }
    if (first_bad >= 0) return set_error(first_rc, "image %d: %s", first_bad, first_msg);
    return GAMUT_HIP_OK;
}

} // namespace
} // namespace gamut

using namespace gamut;

extern "C" {

int gamut_hip_qoix_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, int channels, const int64_t* out_offset,
                                       uint8_t* out, gamut_hip_qoix_info* info, int* status_host, void* stream)
{
    clear_error();
    const bool grey = (channels == 1 || channels == 2) && qoix_plane_on();
    if (count < 0 || (channels != 0 && channels != 3 && channels != 4 && !grey) || (count > 0 && (!data || !len || !out_offset || !out)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "qoix_decode_batch_device: bad arguments (channels is 0, 3 or 4; 1 or 2 with gamut_hip_qoix_set_plane(1))");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return decode_batch(data, len, count, channels, out_offset, out, info, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "qoix_decode_batch_device: out of host memory");
    }
}

// qoix_lz4_decode (plugins/qoix.d:350-473) with the reference's argument list: the file's own channel count, tight rows, malloc'd
void* gamut_hip_qoix_lz4_decode(const void* data, int size, gamut_hip_qoix_info* info, int flags, int* decoded_type)
{
    clear_error();
    gamut_hip_qoix_info qi;
    if (decoded_type) *decoded_type = -1;
    if (!data || size < 0) { set_error(GAMUT_HIP_ERR_INVALID_ARG, "qoix_lz4_decode: bad arguments"); return nullptr; }
    if (size >= (int)kHeader && !gamut_valid_load_flags(flags)) { qoix_fail("invalid load flags"); return nullptr; }          // :359
    const int hrc = qoix_parse_header((const uint8_t*)data, (size_t)size, &qi, nullptr);
    if (info) *info = qi;
    if (hrc != GAMUT_HIP_OK) return nullptr;
    if (!have_device()) return nullptr;
    const size_t nbytes = (size_t)(uint32_t)qi.width * (uint32_t)qi.height * (size_t)qi.channels;
    static thread_local PerDevice<DeviceScratch> out_pd;
    hipStream_t st = thread_stream();
    uint8_t* dev = (uint8_t*)out_pd.cur().get(nbytes, st);
    uint8_t* res = (uint8_t*)malloc(nbytes);
    if (!dev || !res) { free(res); set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "qoix_lz4_decode: %zu bytes", nbytes); return nullptr; }
    const uint8_t* bytes = (const uint8_t*)data; const size_t len = (size_t)size; const int64_t zero = 0; int status = 0;
    int rc;
    try { rc = decode_batch(&bytes, &len, 1, 0, &zero, dev, nullptr, &status, st); }
    catch (...) { rc = set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "qoix_lz4_decode: out of host memory"); }
    if (rc == GAMUT_HIP_OK && (hipMemcpyAsync(res, dev, nbytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) {
        (void)hipGetLastError();
        rc = set_error(GAMUT_HIP_ERR_HIP, "qoix_lz4_decode: copying the pixels back failed");
    }
    if (rc != GAMUT_HIP_OK) { free(res); return nullptr; }
    if (decoded_type) *decoded_type = qi.pixel_type;                           // decodedType = streamType :458-459
    return res;
}

int gamut_hip_qoix_row_capacity(void) { return (int)kRowCap; }
int gamut_hip_qoix_plane_row_capacity(void) { return (int)kPlaneCap; }

float gamut_hip_qoix_last_decode_kernel_ms(void) { return t_last_ms[0] < 0 || t_last_ms[1] < 0 ? -1.0f : t_last_ms[0] + t_last_ms[1]; }
float gamut_hip_qoix_last_decode_stage_ms(int stage) { return stage == 0 || stage == 1 ? t_last_ms[stage] : -1.0f; }
float gamut_hip_qoix_last_plane_kernel_ms(void) { return t_last_ms[2]; }

} // extern "C"
