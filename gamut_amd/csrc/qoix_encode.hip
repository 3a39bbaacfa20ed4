// qoix_encode.hip -- QOIX 8-bit files on the GPU, colour and (behind the QOI-Plane switch) grey: the bytes of qoix_lz4_encode (source/gamut/plugins/qoix.d:251-339) as saveQOIX
// drives it (:156-242) for 8-bit rgb / rgba, that is the QOI2AVG op stream of qoix_encode (source/gamut/codecs/qoi2avg.d:376-615), the
// LZ4 block of LZ4_compress on a 64-bit build (source/gamut/codecs/lz4.d:289-554) and the rule that the smaller file wins, many images
// per call.
//
// The file.  25 header bytes ("qoix", width and height big-endian, version 1, channels, bitdepth 8, colorspace, compression, the two
// floats big-endian bit for bit), then either the op stream and four 0xff bytes (compression 0), or the length of those as a
// big-endian int and their LZ4 block (compression 1), which is chosen when lz4Size + 4 < datalen.
//
// What is parallel and what is not.  In an encoder the left pixel, the row above and the pixel above-left are input, so "repeats its
// predecessor", the alpha step, the LOCO-I reference colour and the colour op with its bytes are functions of the source alone: a
// wave takes 64 pixels of the raster at a time and every lane computes all of that for its pixel.  Where a run is cut (at 1024, at a
// pixel that differs, at the last pixel) follows from the distance to the last pixel that differed, a prefix maximum on one ballot.
// The one chain is the index.  Its two tables are not kept: a pixel hits exactly when the last pixel of its hash (hit or miss) has
// its value and fewer than 65 misses lie between the miss that heads that chain of equal values and the pixel (see encode_group), so
// per hash the wave keeps that last value and the head's miss number in LDS.  A pixel whose hash is alone in its group of 64 and
// whose value differs from the remembered one is a miss whatever came before; only the others are judged in order, with wave-uniform
// values -- a handful per group on photo-like content.  Byte positions are a prefix sum over the lanes (three ballots: a pixel
// writes at most 7 bytes); the bytes are assembled in the wave's LDS and leave as aligned 16-byte pieces (flush_run).
//
// LZ4 is serial per stream: a wave per stream, the 16 KiB table in LDS (8192 x 16 bit below 65547 input bytes, 4096 x 32 bit from
// there).  The search takes 64 attempts at a time -- attempt t of a search looks at ip + F(t), F the closed form of the reference's
// growing step -- each lane fetches its sequence, its table entry and the candidate's sequence, then the attempts are judged in order
// with uniform values, every judged attempt storing its position and patching the later lanes' candidates that share its hash, so
// the table's state at every attempt is the serial one.  Catch-up, match counting, the 255-runs of long lengths and the literal
// copies run across the lanes.  Every loop consumes input or produces output.
//
// Three launches on the call's stream, whatever the batch holds:
//   k_qxenc_ops   a wave per image: header, ops and pad -- straight into the output for mode 1, into scratch for mode 0;
//   k_qxenc_lz4   a wave per mode-0 image: the LZ4 block of the ops, behind a copy of the header with compression 1 and the length;
//   k_qxenc_pick  mode-0 images: the smaller candidate goes to the output (scratch slots are congruent to their destination modulo
//                 16: a byte head and tail, 16-byte pieces between).
// Nothing outside [out_offset, out_offset + out_len) is written.
//
// Grey: 1 or 2 channels are QOI-Plane (qoiplane_encode, source/gamut/codecs/qoiplane.d:109-365), accepted while the process-wide switch
// of qoix_host.hip is on (gamut_hip_qoix_set_plane / GAMUT_HIP_QOIX_PLANE: "the QOI-Plane codec is on", in both directions); off, such a
// description is refused as before the codec existed.  The ops sit on nibble boundaries, high nibble first; the state starts as
// {l: 0, a: 255}; a run is cut at 258 pixels, at the image's last pixel and in front of a pixel that differs.  This encoder has no
// serial chain at all: the predecessor, the pixel above and the run count are input, so an image is cut into segments of kSeg
// consecutive pixels of the raster (whatever the width is) and a wave takes a segment 64 pixels at a time.  Only the distance to the
// last pixel that differed, modulo 258, crosses a segment boundary.  Three more launches, whatever the batch's grey images are:
//   k_qpenc_count  a wave per segment: the repeats in front of its first differing pixel, that pixel's place (or none), the nibbles of
//                  everything behind the leading stretch and the last of them.  What the leading stretch emits is a closed form of
//                  its length and the entering run count e (qp_lead), so it is left to the scan;
//   k_qpenc_scan   a wave per image over its segments, 64 at a time: e (a prefix maximum of the last differing pixel), the first
//                  nibble (a prefix sum), the nibble in front of it (a prefix "last that exists") and the image's stored length;
//   k_qpenc_write  a wave per segment: the ops again, OR-ed as nibbles into the zeroed LDS stage (ds atomics on the stage only) and out
//                  through flush_run.  Byte ownership is fixed: a segment that starts on an odd nibble writes the shared byte whole
//                  (the carried nibble high, its own first low), one that ends on an odd nibble leaves its half byte to the next
//                  segment that emits; the segment with the last pixel writes the closing nibbles, the first one the header.
// k_qxenc_lz4 and k_qxenc_pick then serve grey and colour images alike.  A batch without grey images issues the three launches above,
// one without colour images does not launch k_qxenc_ops.
//
// The bound.  The stored stream behind the header has at most datalen_max = (w * h * n + 10) / 2 bytes, n = 3 nibbles a pixel for 1
// channel and 6 for 2: the ops, the nine closing nibbles and one more to end on a byte.  The bound is 29 + datalen_max +
// datalen_max / 255 + 16, as for colour.
//
// DELIBERATE DEVIATIONS.
//   1. For 4 channels the reference copies pitchBytes into a scanline buffer of 4 * width bytes: a padded pitch overruns it, a negative
//      one is a huge memcpy.  Here width * channels bytes of every row are read, whatever the pitch is.
//   2. The reference's int max_size wraps for large shapes; a description whose bound exceeds 2^31 - 1 is refused instead.
//   G1. qoiplane_encode allocates (w * h * n + 1) / 2 + 29 bytes, one too few whenever every pixel takes its worst op and w * h * n is
//       even (1 x n images alternating 100 / 200, n = 1..39: all 39 two-channel shapes and the 19 even one-channel ones overrun it;
//       tests/test_qoix_plane_encode_cpu.py).  The file's content is well defined all the same; the bound here is the true maximum.
//   G2. w * h * 6 above 2^31 - 1 (2 channels, more than 357913941 pixels) is refused: the reference's int size wraps there.
//   Padded and negative pitches are honoured as the reference honours them for grey: width * channels bytes of a row are read.
#include "encode_host.hpp"
#include "device_util.hpp"

namespace gamut {

bool qoix_plane_on();                                                        // qoix_host.hip: gamut_hip_qoix_set_plane / GAMUT_HIP_QOIX_PLANE

namespace {

constexpr int kWave = 64;
constexpr uint32_t kHeader = 25;
constexpr uint32_t kFlushAt = 2048;                                          // bytes assembled in LDS between two flushes
constexpr uint32_t kStageDwords = (kFlushAt + 7 * kWave) / 4 + 8;            // + one group's worst case, spare dwords for flush_run
constexpr uint32_t kPixelsMax = 400000000u;
constexpr int kPickBlocks = 32, kPickThreads = 256;
constexpr int kAhead = 4;                                                    // groups of 64 pixels fetched ahead
constexpr uint32_t kLz64K = 65547u, kLzMaxInput = 0x7E000000u;
constexpr uint32_t kSeg = 4096;                                              // QOI-Plane: pixels of a segment, a multiple of 64 whatever the width is
constexpr uint32_t kRunMax = 258, kNoNibble = 0xffu;
constexpr uint32_t kQpFlushAt = 2048;                                        // bytes assembled in LDS between two flushes
constexpr uint32_t kQpStageDwords = (kQpFlushAt + 9 * kWave / 2) / 4 + 8;    // + one group's worst case (9 nibbles a pixel), spare dwords for flush_run

struct QeImg {
    const uint8_t* src; int64_t pitch;
    uint8_t* dst;                                                            // byte 0 of the stored file: the output (mode 1) or its scratch slot
    uint32_t w, h, par, dpi;
    uint8_t  ch, cs, pad0, pad1;
    uint32_t slot;                                                           // index of the image's length words
};
struct LzJob {
    const uint8_t* src; uint8_t* dst;                                        // header 1: a stored file and a candidate file; 0: bytes and block
    uint32_t len, header, slot, pad;                                         // header 1: the length is file_len[slot] - 25
};
struct QpImg { QeImg im; uint32_t seg0, nseg; };                            // a grey image and the number of its first segment in the batch
struct QpSeg {                                                               // k_qpenc_count, per segment
    int32_t last_diff;                                                       // the last pixel (raster index) that differs from its predecessor, -1: none
    uint32_t lead, rest, rest_last;                                          // repeats in front of the first such pixel; nibbles behind them, the last of those
};
struct QpPlace { uint32_t e, off, carry, pad; };                             // k_qpenc_scan: entering run count, first nibble, the nibble in front of it
struct PickJob { const uint8_t* stored; const uint8_t* cand; uint8_t* dst; uint32_t slot, pad; };

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t rdl(uint32_t v, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane); }
__device__ __forceinline__ void wave_order() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }   // (compiler order only: one wave's LDS and global accesses are served in issue order)

// LOCO-I per channel from left a, up b, up-left c (qoi2avg.d:843-897), as k_qoix_avg holds it
__device__ __forceinline__ uint32_t loco1(uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t mx = max(a, b), mn = min(a, b);
    uint32_t p = a + b - c;
    if (c >= mx) p = mn;
    if (c <= mn) p = mx;
    return p & 255u;
}

// a pixel as r | g << 8 | b << 16 | a << 24 (255 without an alpha channel), by bytes and without a branch: the loads of a fetch are
// one straight line, so that they stay in flight while the groups in front are encoded
__device__ __forceinline__ uint32_t load_px(const uint8_t* p, uint32_t ch)
{
    const uint32_t b0 = p[0], b1 = p[1], b2 = p[2], b3 = p[ch - 1];
    return b0 | b1 << 8 | b2 << 16 | (ch == 4 ? b3 : 255u) << 24;
}

// the two bytes of RUN2 for `run` + 1 pixels, low byte first in the result
__device__ __forceinline__ uint32_t run2(uint32_t run) { return (0xf8u | ((run >> 8) & 3u)) | (run & 255u) << 8; }

// What a pixel that missed the index writes (:508-591): bytes in emission order from bit 0, the count in *len.
__device__ __forceinline__ uint64_t miss_op(uint32_t v, uint32_t prev, uint32_t up, uint32_t ul, bool row0, bool col0, uint32_t* len)
{
    const uint32_t r = v & 255u, g = (v >> 8) & 255u, b = (v >> 16) & 255u, a = v >> 24;
    const int va = (int8_t)(a - (prev >> 24));
    uint64_t out = 0; uint32_t n = 0;
    if (va) {
        if (va < -4 || va > 3) { *len = 5; return 0xfeull | (uint64_t)v << 8; }
        out = 0xe8u | (uint32_t)(va + 4); n = 1;
    }
    uint32_t rr = prev & 255u, rg = (prev >> 8) & 255u, rb = (prev >> 16) & 255u;
    if (!row0) {
        if (col0) { rr = up & 255u; rg = (up >> 8) & 255u; rb = (up >> 16) & 255u; }
        else {
            rr = loco1(rr, up & 255u, ul & 255u); rg = loco1(rg, (up >> 8) & 255u, (ul >> 8) & 255u); rb = loco1(rb, (up >> 16) & 255u, (ul >> 16) & 255u);
        }
    }
    const int vg = (int8_t)(g - rg), vr = (int8_t)(r - rr - (uint32_t)vg), vb = (int8_t)(b - rb - (uint32_t)vg);
    uint32_t op, m;
    if (vg >= -4 && vg < 0 && vr >= -1 && vr <= 2 && vb >= -1 && vb <= 2) { op = (uint32_t)((vg + 4) << 4 | (vr + 1) << 2 | (vb + 1)); m = 1; }
    else if (vg >= 0 && vg <= 3 && vr >= -2 && vr <= 1 && vb >= -2 && vb <= 1) { op = (uint32_t)((vg + 4) << 4 | (vr + 2) << 2 | (vb + 2)); m = 1; }
    else if (g == r && g == b) { op = 0xfcu | g << 8; m = 2; }
    else if (vr >= -8 && vr <= 7 && vg >= -16 && vg <= 15 && vb >= -8 && vb <= 7) { op = (0xc0u | (uint32_t)(vg + 16)) | (uint32_t)((vr + 8) << 4 | (vb + 8)) << 8; m = 2; }
    else if (vr >= -32 && vr <= 31 && vg >= -64 && vg <= 63 && vb >= -32 && vb <= 31) {
        const uint32_t dv = (uint32_t)((vg + 64) << 12 | (vr + 32) << 6 | (vb + 32));
        op = (0xe0u | ((dv >> 16) & 31u)) | ((dv >> 8) & 255u) << 8 | (dv & 255u) << 16; m = 3;
    } else { op = 0xfdu | (v & 0xFFFFFFu) << 8; m = 4; }
    *len = n + m;
    return out | (uint64_t)op << (8 * n);
}

__global__ void __launch_bounds__(kWave) k_qxenc_ops(const QeImg* __restrict__ imgs, uint32_t* __restrict__ file_len)
{
    __shared__ uint32_t tval[1024];                                          // per hash: the last pixel that differed from its predecessor
    __shared__ int32_t thead[1024];                                          // ... and the number of the miss that heads its chain of equal values
    __shared__ uint8_t owner[1024];                                          // a lane of the current group per hash
    __shared__ uint32_t stage[kStageDwords];
    const QeImg im = imgs[blockIdx.x];
    const uint32_t lane = threadIdx.x, w = im.w, ch = im.ch, total = im.w * im.h;
    const uint64_t lt = (1ull << lane) - 1;
    uint8_t* Sb = reinterpret_cast<uint8_t*>(stage);
    for (uint32_t k = lane; k < 1024; k += kWave) { tval[k] = 0; thead[k] = -64; }
    if (lane < kHeader) {                                                    // :421-430
        const uint32_t word = lane < 4 ? 0x716F6978u : lane < 8 ? w : lane < 12 ? im.h : lane < 21 ? im.par : im.dpi;
        const uint32_t pos = lane < 12 ? lane & 3u : lane < 17 ? 0u : (lane - 17u) & 3u;
        uint32_t b = (word >> (24u - 8u * pos)) & 255u;
        if (lane >= 12 && lane < 17) b = lane == 12 ? 1u : lane == 13 ? ch : lane == 14 ? 8u : lane == 15 ? im.cs : 0u;
        Sb[lane] = (uint8_t)b;
    }
    const uint32_t groups = (total + kWave - 1) / kWave;
    const uint64_t magic = w > 1 ? ~0ull / w + 1 : 0;                        // i / w = the high half of i * magic for every i < 2^32
    auto row_of = [&](uint32_t i) -> uint32_t { return w > 1 ? (uint32_t)__umul64hi((uint64_t)i, magic) : i; };
    // kAhead groups at a time: the lanes' pixels and the pixels above them, asked for while the kAhead groups in front are encoded.
    // Positions behind the image read its last pixel and row 0 reads itself as the row above: every address is inside the image.
    auto fetch = [&](uint32_t g0, uint32_t* v, uint32_t* up) {
        #pragma unroll
        for (int q = 0; q < kAhead; ++q) {
            const uint32_t i = min((g0 + q) * kWave + lane, total - 1), y = row_of(i), x = i - y * w;
            const uint8_t* p = im.src + (int64_t)y * im.pitch + (size_t)x * ch;
            v[q] = load_px(p, ch);
            up[q] = load_px(y > 0 ? p - im.pitch : p, ch);
        }
    };
    uint32_t last_v = 0xFF000000u, last_up = 0;                              // px starts as (0, 0, 0, 255)
    int64_t last_diff = -1;                                                  // the last pixel that differed from its predecessor
    uint32_t misses = 0, fill = kHeader, written = 0;
    auto encode_group = [&](uint32_t g, uint32_t v, uint32_t up) {
        const uint32_t i = g * kWave + lane, y = row_of(i), x = i - y * w;
        const bool valid = i < total;
        uint32_t prev = __shfl_up(v, 1, kWave), ul = __shfl_up(up, 1, kWave);
        if (lane == 0) { prev = last_v; ul = last_up; }
        const bool diff = valid && v != prev;
        const uint64_t D = __ballot(diff);
        const uint32_t hash = ((v * 2654435769u) >> 22) & 1023u;
        uint32_t oplen = 0;
        uint64_t op = 0;
        if (diff) op = miss_op(v, prev, up, ul, y == 0, x == 0, &oplen);
        // the index :486-506, without its two tables.  index_lookup[hash] is the slot of the last MISS with that hash, and the slot still
        // holds that pixel until 64 further misses have passed (a miss that overwrote it with an equal pixel would own the hash
        // entry).  So with c misses in front of it, a pixel hits exactly when the last pixel of its hash that differed from its
        // predecessor (hit or miss) carries the same value and the miss that heads that chain of equal values has a number >=
        // c - 64; the INDEX it writes is that number modulo 64.  Per hash: tval = that last value, thead = its chain head's number;
        // zero and -64 at first, which is the all-zero state (a pixel (0,0,0,0) hits until the first miss).  A pixel whose hash
        // nobody else in the group has and whose value differs from tval is a miss whatever came before: only the others (Wm)
        // are judged in order, with uniform values, each patching the lanes of its hash.
        uint32_t hit_at = 0;
        uint64_t hits = 0;
        if (D) {                                                             // (uniform over the wave)
        wave_order();
        uint32_t tv = 0; int32_t th = 0;
        if (diff) { tv = tval[hash]; th = thead[hash]; owner[hash] = (uint8_t)lane; }
        wave_order();
        const bool loser = diff && owner[hash] != lane;
        wave_order();
        if (loser) owner[hash] = 0xFF;
        wave_order();
        const bool walked = diff && (owner[hash] == 0xFF || tv == v);
        for (uint64_t m = __ballot(walked); m; m &= m - 1) {                 // (uniform over the wave)
            const uint32_t j = (uint32_t)__builtin_ctzll(m), vj = rdl(v, j), tvj = rdl(tv, j), hj = rdl(hash, j);
            const int32_t thj = (int32_t)rdl((uint32_t)th, j);
            const int32_t cj = (int32_t)(misses + (uint32_t)__builtin_popcountll(D & ((1ull << j) - 1)) - (uint32_t)__builtin_popcountll(hits));
            if (tvj == vj && cj - thj <= 64) {
                hits |= 1ull << j;
                if (lane == j) hit_at = (uint32_t)thj & 63u;
            } else if (hash == hj) { tv = vj; th = cj; }
        }
        if (diff && !walked) { tv = v; th = (int32_t)(misses + (uint32_t)__builtin_popcountll(D & lt) - (uint32_t)__builtin_popcountll(hits & lt)); }
        if (diff) { tval[hash] = tv; thead[hash] = th; }
        misses += (uint32_t)__builtin_popcountll(D) - (uint32_t)__builtin_popcountll(hits);
        if ((hits >> lane) & 1u) { op = 0x80u | hit_at; oplen = 1; }
        wave_order();
        }
        // the runs: k pixels since the last one that differed, this one included
        const uint64_t below = D & lt;
        const int64_t ld = below ? (int64_t)(g * kWave) + (63 - __builtin_clzll(below)) : last_diff;
        const uint32_t k = (uint32_t)((int64_t)i - ld);
        uint64_t bytes = 0; uint32_t n = 0;
        if (diff) {
            const uint32_t pending = (k - 1) & 1023u;                        // :488-498
            if (pending) {
                if (pending <= 8) { bytes = 0xf0u | (pending - 1); n = 1; }
                else { bytes = run2(pending - 1); n = 2; }
            }
            bytes |= op << (8 * n); n += oplen;
        } else if (valid) {
            if ((k & 1023u) == 0) { bytes = run2(1023); n = 2; }             // :478-483
            else if (i == total - 1) { bytes = run2((k & 1023u) - 1); n = 2; }
        }
        const uint64_t n0 = __ballot(n & 1u), n1 = __ballot(n & 2u), n2 = __ballot(n & 4u);       // n <= 7: a prefix sum on three ballots
        const uint32_t off = fill + (uint32_t)__builtin_popcountll(n0 & lt) + 2u * (uint32_t)__builtin_popcountll(n1 & lt) + 4u * (uint32_t)__builtin_popcountll(n2 & lt);
        for (uint32_t q = 0; q < n; ++q) Sb[off + q] = (uint8_t)(bytes >> (8 * q));
        fill += (uint32_t)__builtin_popcountll(n0) + 2u * (uint32_t)__builtin_popcountll(n1) + 4u * (uint32_t)__builtin_popcountll(n2);
        if (D) last_diff = (int64_t)(g * kWave) + (63 - __builtin_clzll(D));
        last_v = rdl(v, kWave - 1); last_up = rdl(up, kWave - 1);
        if (fill >= kFlushAt) {
            wave_order(); flush_run<kWave>(stage, im.dst + written, fill, lane); wave_order();
            written += fill; fill = 0;
        }
    };
    uint32_t cv[kAhead], cu[kAhead], nv[kAhead], nu[kAhead];
    fetch(0, cv, cu);
    for (uint32_t g0 = 0; g0 < groups; g0 += kAhead) {
        fetch(g0 + kAhead, nv, nu);                                          // (nothing is loaded behind the image)
        #pragma unroll
        for (int q = 0; q < kAhead; ++q) if (g0 + q < groups) encode_group(g0 + q, cv[q], cu[q]);
        #pragma unroll
        for (int q = 0; q < kAhead; ++q) { cv[q] = nv[q]; cu[q] = nu[q]; }
    }
    if (lane < 4) Sb[fill + lane] = 0xff;                                    // :608-611
    fill += 4;
    wave_order(); flush_run<kWave>(stage, im.dst + written, fill, lane);
    if (lane == 0) file_len[im.slot] = written + fill;
}

// ---- QOI-Plane (qoiplane.d:109-365) -------------------------------------------------------------------------------------------------

// The op nibbles of a pixel v = l | a << 8 that differs from its predecessor `prev` (:257-306), first nibble in bits 0..3, the count in
// *len (at most 6).  `top` is channel 0 of the pixel above, prev's in row 0.
__device__ __forceinline__ uint32_t qp_op(uint32_t v, uint32_t prev, uint32_t top, uint32_t* len)
{
    const uint32_t l = v & 255u, a = v >> 8, rl = prev & 255u;
    const int va = (int8_t)(a - (prev >> 8));
    uint32_t out = 0, n = 0;
    if (va) {
        if (va < -7 || va > 7) { *len = 6; return 0xbu | (l >> 4) << 8 | (l & 15u) << 12 | (a >> 4) << 16 | (a & 15u) << 20; }       // LA
        out = 0xbu | (uint32_t)(va + 8) << 4; n = 2;                          // ADIFF
    }
    const int d = (int8_t)(l - ((top + rl + 1u) >> 1));
    uint32_t op, m;
    if (d >= -4 && d <= 3) { op = (uint32_t)(d + 4); m = 1; }
    else if (d >= -16 && d <= 15) { const uint32_t b = 0x80u | (uint32_t)(d + 16); op = b >> 4 | (b & 15u) << 4; m = 2; }
    else { op = 0xau | (l >> 4) << 4 | (l & 15u) << 8; m = 3; }
    *len = n + m;
    return out | op << (4 * n);
}

// encodeRun :191-216 for 1..258 pixels, as nibbles
__device__ __forceinline__ uint32_t qp_run(uint32_t run, uint32_t* len)
{
    if (run <= 3) { *len = 1; return 0xcu | (run - 1); }
    *len = 3;
    return 0xfu | ((run - 4) >> 4) << 4 | ((run - 4) & 15u) << 8;
}

// What the repeats in front of a segment's first differing pixel emit, as a function of their number `lead` and of the run count
// `e` (0..257) that enters the segment: a REPEAT2 of 258 whenever the count gets there, and the rest when the stretch ends at a pixel
// that differs or at the image's last pixel (`closed`).  Returns the nibble count; *last is the last nibble, kNoNibble when none.
__device__ __forceinline__ uint32_t qp_lead(uint32_t e, uint32_t lead, bool closed, uint32_t* last)
{
    const uint32_t t = e + lead, full = t / kRunMax, r = t - full * kRunMax;
    uint32_t n = 3 * full;
    *last = full ? 0xeu : kNoNibble;                                         // f f e: 258 - 4
    if (closed && r) { uint32_t m; const uint32_t nib = qp_run(r, &m); n += m; *last = (nib >> (4 * (m - 1))) & 15u; }
    return n;
}

// A segment of the raster, 64 pixels at a time: every lane computes its pixel's predecessor, the pixel above and its nibbles from the
// source.  kWrite false (k_qpenc_count): what lies behind the leading repeats is counted, the first differing pixel without the run
// in front of it (that run belongs to the leading stretch, whose emission depends on e).  kWrite true (k_qpenc_write): e is known,
// so the leading stretch is like any other; the nibbles are OR-ed into the zeroed LDS stage and leave through flush_run.
template <bool kWrite> __device__ __forceinline__ void qp_segment(const QpImg& qi, uint32_t seg, QpSeg* rec, const QpPlace* place, uint32_t* stage)
{
    const QeImg& im = qi.im;
    const uint32_t lane = threadIdx.x, w = im.w, ch = im.ch, total = im.w * im.h;
    const uint64_t lt = (1ull << lane) - 1;
    const uint32_t s0 = seg * kSeg, s1 = min(total, s0 + kSeg);
    const bool holds_last = s1 == total;
    const uint64_t magic = w > 1 ? ~0ull / w + 1 : 0;                        // i / w = the high half of i * magic for every i < 2^32
    auto row_of = [&](uint32_t i) -> uint32_t { return w > 1 ? (uint32_t)__umul64hi((uint64_t)i, magic) : i; };
    auto pixel = [&](uint32_t i, uint32_t* top) -> uint32_t {               // i < total: every address is inside the image
        const uint32_t y = row_of(i), x = i - y * w;
        const uint8_t* p = im.src + (int64_t)y * im.pitch + (size_t)x * ch;
        *top = y > 0 ? (uint32_t)*(p - im.pitch) : 256u;                     // 256: row 0, the predecessor stands in
        return p[0] | (ch == 2 ? (uint32_t)p[1] : 255u) << 8;
    };
    uint32_t dummy;
    uint32_t last_v = s0 ? rfl(pixel(s0 - 1, &dummy)) : 0xFF00u;             // the state starts as {l: 0, a: 255}
    int32_t ld;                                                              // the last pixel that differed, or what stands for it
    bool seen = kWrite;
    uint32_t fill = 0, written = 0, lead = 0, rest = 0, rest_last = kNoNibble;
    uint8_t* dst = im.dst;
    if (kWrite) {
        const QpPlace pl = place[qi.seg0 + seg];
        ld = (int32_t)s0 - 1 - (int32_t)pl.e;
        for (uint32_t k = lane; k < kQpStageDwords; k += kWave) stage[k] = 0;
        wave_order();
        if (seg == 0) {
            if (lane < kHeader) {                                            // :151-160
                const uint32_t word = lane < 4 ? 0x716F6978u : lane < 8 ? w : lane < 12 ? im.h : lane < 21 ? im.par : im.dpi;
                const uint32_t pos = lane < 12 ? lane & 3u : lane < 17 ? 0u : (lane - 17u) & 3u;
                uint32_t b = (word >> (24u - 8u * pos)) & 255u;
                if (lane >= 12 && lane < 17) b = lane == 12 ? 1u : lane == 13 ? ch : lane == 14 ? 8u : lane == 15 ? im.cs : 0u;
                reinterpret_cast<uint8_t*>(stage)[lane] = (uint8_t)b;
            }
            fill = 2 * kHeader;
        } else {
            dst += kHeader + (pl.off >> 1);
            if (pl.off & 1u) {                                               // the byte shared with the segment in front is written here, whole
                if (lane == 0) stage[0] = (pl.carry & 15u) << 4;
                fill = 1;
            }
        }
        wave_order();
    } else ld = -1;
    uint32_t top_n = 0, v_n = pixel(min(s0 + lane, total - 1), &top_n);
    for (uint32_t i0 = s0; i0 < s1; i0 += kWave) {
        const uint32_t v = v_n, top = top_n;
        if (i0 + kWave < s1) v_n = pixel(min(i0 + kWave + lane, total - 1), &top_n);       // asked for while this group is encoded
        const uint32_t i = i0 + lane;
        const bool valid = i < s1;
        uint32_t prev = __shfl_up(v, 1, kWave);
        if (lane == 0) prev = last_v;
        const bool diff = valid && v != prev;
        const uint64_t D = __ballot(diff);
        const uint64_t below = D & lt;
        const bool known = seen || below;                                    // a pixel that differed lies in front, in this segment or (kWrite) by e
        const uint32_t k = (uint32_t)((int32_t)i - (below ? (int32_t)i0 + (63 - __builtin_clzll(below)) : ld));
        uint64_t nib = 0; uint32_t n = 0;
        if (diff) {
            const uint32_t pending = (k - 1) % kRunMax;                      // :254-255
            if (known && pending) nib = qp_run(pending, &n);
            uint32_t m;
            const uint32_t op = qp_op(v, prev, top > 255u ? prev & 255u : top, &m);
            nib |= (uint64_t)op << (4 * n); n += m;
        } else if (valid && known) {                                         // :246-251
            const uint32_t r = k % kRunMax;
            if (r == 0) nib = qp_run(kRunMax, &n);
            else if (i == total - 1) nib = qp_run(r, &n);
        }
        const uint64_t n0 = __ballot(n & 1u), n1 = __ballot(n & 2u), n2 = __ballot(n & 4u), n3 = __ballot(n & 8u);     // n <= 9
        const uint32_t sum = (uint32_t)__builtin_popcountll(n0) + 2u * (uint32_t)__builtin_popcountll(n1) + 4u * (uint32_t)__builtin_popcountll(n2) +
                             8u * (uint32_t)__builtin_popcountll(n3);
        if (kWrite) {
            uint32_t q = fill + (uint32_t)__builtin_popcountll(n0 & lt) + 2u * (uint32_t)__builtin_popcountll(n1 & lt) +
                         4u * (uint32_t)__builtin_popcountll(n2 & lt) + 8u * (uint32_t)__builtin_popcountll(n3 & lt);
            uint32_t cur = q >> 3, acc = 0;                                  // nibble q: byte q / 2, high half when q is even
            for (uint32_t j = 0; j < n; ++j, ++q) {
                if ((q >> 3) != cur) { atomicOr(&stage[cur], acc); acc = 0; cur = q >> 3; }
                acc |= (uint32_t)((nib >> (4 * j)) & 15u) << (8u * ((q >> 1) & 3u) + ((q & 1u) ? 0u : 4u));
            }
            if (n) atomicOr(&stage[cur], acc);
            fill += sum;
            if (fill >= 2 * kQpFlushAt) {                                    // whole bytes leave; a half byte stays as the stage's first
                const uint32_t bytes = fill >> 1, used = (fill + 7) >> 3;
                wave_order(); flush_run<kWave>(stage, dst + written, bytes, lane); wave_order();
                const uint32_t half = (fill & 1u) ? byte_of(stage, bytes) : 0u;
                wave_order();
                for (uint32_t d = lane; d < used; d += kWave) stage[d] = 0;
                wave_order();
                if (lane == 0) stage[0] = half;
                wave_order();
                written += bytes; fill &= 1u;
            }
        } else {
            if (!seen) lead = D ? i0 - s0 + (uint32_t)__builtin_ctzll(D) : s1 - s0;
            rest += sum;
            const uint64_t any = __ballot(n != 0);
            if (any) { const uint32_t j = 63 - (uint32_t)__builtin_clzll(any); rest_last = (uint32_t)(rdl((uint32_t)(nib >> (4 * (rdl(n, j) - 1))), j)) & 15u; }
        }
        if (D) { ld = (int32_t)i0 + (63 - __builtin_clzll(D)); seen = true; }
        last_v = rdl(v, kWave - 1);
    }
    if (kWrite) {
        if (holds_last) {                                                    // :313-317: nine f nibbles, one more to end on a byte
            const uint32_t closing = 9 + ((fill + 9) & 1u), q = fill + lane;
            wave_order();
            if (lane < closing) atomicOr(&stage[q >> 3], 15u << (8u * ((q >> 1) & 3u) + ((q & 1u) ? 0u : 4u)));
            fill += closing;
        }
        // a segment that emitted nothing writes nothing; one that ends on a half byte leaves it to the next that emits
        wave_order();
        flush_run<kWave>(stage, dst + written, fill >> 1, lane);
    } else if (lane == 0) {
        rec[qi.seg0 + seg] = QpSeg{ seen ? ld : -1, lead, rest, rest_last };
    }
}

__global__ void __launch_bounds__(kWave) k_qpenc_count(const QpImg* __restrict__ imgs, int n_imgs, QpSeg* __restrict__ segs)
{
    const QpImg qi = imgs[find_unit<&QpImg::seg0>(imgs, n_imgs, blockIdx.x)];
    qp_segment<false>(qi, blockIdx.x - qi.seg0, segs, nullptr, nullptr);
}

// A wave per image over its segments, 64 at a time: the run count that enters a segment is its distance to the last pixel that
// differed (a prefix maximum) modulo 258; with it the leading stretch's nibbles are known, and a prefix sum gives every segment its
// first nibble; the last nibble in front of it (a prefix "last one that exists") completes a shared byte.
__global__ void __launch_bounds__(kWave) k_qpenc_scan(const QpImg* __restrict__ imgs, const QpSeg* __restrict__ segs, QpPlace* __restrict__ place,
                                                     uint32_t* __restrict__ file_len)
{
    const QpImg qi = imgs[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    int32_t run_ld = -1;
    uint32_t run_off = 0, run_last = kNoNibble;
    for (uint32_t base = 0; base < qi.nseg; base += kWave) {
        const uint32_t s = base + lane;
        const bool valid = s < qi.nseg;
        const QpSeg rec = valid ? segs[qi.seg0 + s] : QpSeg{ -1, 0u, 0u, kNoNibble };
        int32_t ldmax = rec.last_diff;
        #pragma unroll
        for (int d = 1; d < kWave; d <<= 1) { const int32_t t = __shfl_up(ldmax, d, kWave); if ((int)lane >= d) ldmax = max(ldmax, t); }
        int32_t before = __shfl_up(ldmax, 1, kWave);
        before = lane == 0 ? run_ld : max(before, run_ld);
        const uint32_t s0 = valid ? s * kSeg : 0u;
        const uint32_t e = valid ? (uint32_t)((int32_t)s0 - 1 - before) % kRunMax : 0u;
        uint32_t last;
        uint32_t nib = qp_lead(e, rec.lead, rec.last_diff >= 0 || s + 1 == qi.nseg, &last);
        if (rec.rest) last = rec.rest_last;
        nib += rec.rest;
        if (!valid) { nib = 0; last = kNoNibble; }
        uint32_t sum = nib;
        #pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t t = __shfl_up(sum, d, kWave), tl = __shfl_up(last, d, kWave);
            if ((int)lane >= d) { sum += t; if (last == kNoNibble) last = tl; }
        }
        uint32_t carry = __shfl_up(last, 1, kWave);
        if (lane == 0 || carry == kNoNibble) carry = run_last;
        if (valid) place[qi.seg0 + s] = QpPlace{ e, run_off + sum - nib, carry, 0u };
        run_ld = max(run_ld, (int32_t)rdl((uint32_t)ldmax, kWave - 1));
        run_off += rdl(sum, kWave - 1);
        const uint32_t l63 = rdl(last, kWave - 1);
        if (l63 != kNoNibble) run_last = l63;
    }
    const uint32_t nibbles = run_off + 9u + ((run_off + 9u) & 1u);
    if (lane == 0) file_len[qi.im.slot] = kHeader + (nibbles >> 1);
}

__global__ void __launch_bounds__(kWave) k_qpenc_write(const QpImg* __restrict__ imgs, int n_imgs, const QpPlace* __restrict__ place)
{
    __shared__ uint32_t stage[kQpStageDwords];
    const QpImg qi = imgs[find_unit<&QpImg::seg0>(imgs, n_imgs, blockIdx.x)];
    qp_segment<true>(qi, blockIdx.x - qi.seg0, nullptr, place, stage);
}

// ---- LZ4_compress -----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t rd32(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// where attempt t (1, 2, ...) of a search looks, relative to its first position: step = searchMatchNb++ >> 6 summed (:395-403)
__device__ __forceinline__ uint64_t search_offset(uint64_t t)
{
    if (t <= 1) return 0;
    const uint64_t s = 61 + t, q = s >> 6, r = s & 63u;
    return 1 + 32 * q * (q - 1) + q * (r + 1);
}

// `count` bytes of 255 at dst, then one byte: the tail of a length field whose nibble is 15 (:438-444, :483-490, :533)
__device__ __forceinline__ uint32_t put_length(uint8_t* dst, uint32_t op, uint32_t n, uint32_t lane)
{
    const uint32_t full = n / 255u;
    for (uint32_t k = lane; k < full; k += kWave) dst[op + k] = 255;
    if (lane == 0) dst[op + full] = (uint8_t)(n - full * 255u);
    return op + full + 1;
}

__device__ __forceinline__ void copy_bytes(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t lane)
{
    uint32_t k = 0;
    for (; k + 8 * kWave <= n; k += 8 * kWave) {                             // eight loads in flight per lane
        uint8_t t[8];
        #pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = src[k + q * kWave + lane];
        #pragma unroll
        for (int q = 0; q < 8; ++q) dst[k + q * kWave + lane] = t[q];
    }
    for (k += lane; k < n; k += kWave) dst[k] = src[k];
}

__global__ void __launch_bounds__(kWave) k_qxenc_lz4(const LzJob* __restrict__ jobs, int n_jobs, const uint32_t* __restrict__ file_len,
                                                    uint32_t* __restrict__ lz_len)
{
    __shared__ uint32_t table[4096];                                         // byU32; byU16 keeps 8192 halves in the same bytes
    __shared__ uint8_t owner[8192];                                          // a lane of the current batch of attempts per hash
    if ((int)blockIdx.x >= n_jobs) return;
    const LzJob job = jobs[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    const uint32_t n = job.header ? file_len[job.slot] - kHeader : job.len;
    const uint8_t* src = job.header ? job.src + kHeader : job.src;
    uint8_t* dst = job.header ? job.dst + kHeader + 4 : job.dst;
    const bool u16 = n < kLz64K;
    uint16_t* table16 = reinterpret_cast<uint16_t*>(table);
    for (uint32_t k = lane; k < 4096; k += kWave) table[k] = 0;
    auto hash_of = [&](uint32_t seq) { return (seq * 2654435761u) >> (u16 ? 19 : 20); };
    auto get = [&](uint32_t h) -> uint32_t { return u16 ? table16[h] : table[h]; };
    auto put = [&](uint32_t h, uint32_t pos) { if (u16) table16[h] = (uint16_t)pos; else table[h] = pos; };
    uint32_t ip = 0, anchor = 0, op = 0;
    if (n >= 13) {
        const uint32_t mflimit = n - 12, matchlimit = n - 5;
        wave_order();
        if (lane == 0) put(hash_of(rd32(src)), 0);
        ip = 1;
        for (;;) {
            // the search :399-426, 64 attempts at a time.  An attempt that is judged stores its position; `cand` is kept what the
            // table would hold: where no two attempts of the batch share a hash (owner[] tells) the verdicts do not depend on each
            // other and the first match is one ballot; else the attempts are judged in order, each patching the lanes of its hash.
            uint32_t match = 0;
            bool found = false, over = false;
            for (uint64_t t0 = 1; !found && !over; t0 += kWave) {
                const uint64_t t = t0 + lane, pos64 = ip + search_offset(t);
                const bool ok = ip + search_offset(t + 1) <= mflimit;        // :405 forwardIp > mflimit ends the block
                const uint32_t pos = ok ? (uint32_t)pos64 : 0u;
                const uint32_t seq = ok ? rd32(src + pos) : 0u, h = hash_of(seq);
                wave_order();
                uint32_t cand = ok ? get(h) : 0u;
                if (ok) owner[h] = (uint8_t)lane;
                uint32_t cseq = ok ? rd32(src + cand) : 0u;
                wave_order();
                const bool shared = ok && owner[h] != lane;
                const uint64_t okm = __ballot(ok);                           // (the lanes below some lane: the positions grow)
                const uint32_t n_ok = ~okm ? (uint32_t)__builtin_ctzll(~okm) : (uint32_t)kWave;
                uint32_t judged = n_ok;
                if (__ballot(shared) == 0) {
                    const uint64_t hm = __ballot(ok && (u16 || cand + 65535u >= pos) && cseq == seq);
                    if (hm) { const uint32_t j = (uint32_t)__builtin_ctzll(hm); found = true; ip = rdl(pos, j); match = rdl(cand, j); judged = j + 1; }
                    cand = pos;
                } else {
                    for (uint32_t j = 0; j < n_ok; ++j) {                    // (uniform over the wave)
                        const uint32_t pj = rdl(pos, j), cj = rdl(cand, j), csj = rdl(cseq, j), sj = rdl(seq, j), hj = rdl(h, j);
                        if (h == hj) { cand = pj; cseq = sj; }
                        if ((u16 || cj + 65535u >= pj) && csj == sj) { found = true; ip = pj; match = cj; judged = j + 1; break; }
                    }
                }
                if (lane < judged) put(h, cand);                             // the last judged attempt of every hash
                wave_order();
                over = !found && n_ok < (uint32_t)kWave;                     // an attempt past mflimit
            }
            if (!found) break;
            // catch up :430
            for (;;) {
                const bool c = (int64_t)ip - 1 - lane >= (int64_t)anchor && match >= 1 + lane && src[ip - 1 - lane] == src[match - 1 - lane];
                const uint64_t nm = ~__ballot(c);
                const uint32_t cnt = nm ? (uint32_t)__builtin_ctzll(nm) : (uint32_t)kWave;
                ip -= cnt; match -= cnt;
                if (cnt < (uint32_t)kWave) break;
            }
            // literals :432-450
            const uint32_t lit = ip - anchor;
            uint32_t token_at = op++, token = min(lit, 15u) << 4;
            if (lit >= 15) op = put_length(dst, op, lit - 15, lane);
            copy_bytes(dst + op, src + anchor, lit, lane);
            op += lit;
            for (;;) {                                                       // _next_match :452-521
                if (lane == 0) { dst[op] = (uint8_t)(ip - match); dst[op + 1] = (uint8_t)((ip - match) >> 8); }
                op += 2;
                uint32_t ml = 0;
                for (;;) {                                                   // LZ4_count: common bytes, up to matchlimit
                    const uint32_t a = ip + 4 + ml + lane;
                    const bool c = a < matchlimit && src[match + 4 + ml + lane] == src[a];
                    const uint64_t nm = ~__ballot(c);
                    const uint32_t cnt = nm ? (uint32_t)__builtin_ctzll(nm) : (uint32_t)kWave;
                    ml += cnt;
                    if (cnt < (uint32_t)kWave) break;
                }
                ip += 4 + ml;
                token |= min(ml, 15u);
                if (lane == 0) dst[token_at] = (uint8_t)token;
                if (ml >= 15) op = put_length(dst, op, ml - 15, lane);
                anchor = ip;
                if (ip > mflimit) break;
                wave_order();
                if (lane == 0) put(hash_of(rd32(src + ip - 2)), ip - 2);     // :500
                wave_order();
                const uint32_t seq = rd32(src + ip), h = hash_of(seq);
                match = rfl(get(h));
                wave_order();
                if (lane == 0) put(h, ip);
                if (match + 65535u >= ip && rfl(rd32(src + match)) == rfl(seq)) { token_at = op++; token = 0; continue; }
                break;
            }
            if (ip > mflimit) break;
            ++ip;
        }
    }
    // _last_literals :527-537
    const uint32_t last = n - anchor;
    if (lane == 0) dst[op] = (uint8_t)(min(last, 15u) << 4);
    ++op;
    if (last >= 15) op = put_length(dst, op, last - 15, lane);
    copy_bytes(dst + op, src + anchor, last, lane);
    op += last;
    if (lane == 0) lz_len[job.slot] = op;
    if (job.header && lane < kHeader + 4) {                                  // plugins/qoix.d:306-308, :325
        uint32_t b = lane < kHeader ? job.src[lane] : (n >> (24u - 8u * (lane - kHeader))) & 255u;
        if (lane == 16) b = 1;
        job.dst[lane] = (uint8_t)b;
    }
}

// plugins/qoix.d:319-338: the compressed file when lz4Size + 4 < datalen, else the stored one
__global__ void __launch_bounds__(kPickThreads) k_qxenc_pick(const PickJob* __restrict__ jobs, int n_jobs, const uint32_t* __restrict__ file_len,
                                                            const uint32_t* __restrict__ lz_len, uint32_t* __restrict__ final_len)
{
    if ((int)blockIdx.x >= n_jobs) return;
    const PickJob job = jobs[blockIdx.x];
    const uint32_t stored = file_len[job.slot], lz = lz_len[job.slot];
    const bool packed = lz + 4 < stored - kHeader;
    const uint8_t* src = packed ? job.cand : job.stored;                     // both congruent to dst modulo 16
    const uint32_t n = packed ? kHeader + 4 + lz : stored;
    const uint32_t tid = blockIdx.y * kPickThreads + threadIdx.x, threads = kPickBlocks * kPickThreads;
    const uint32_t head = min(n, (uint32_t)((16u - ((uintptr_t)job.dst & 15u)) & 15u)), chunks = (n - head) >> 4;
    if (tid < head) job.dst[tid] = src[tid];
    for (uint32_t c = tid; c < chunks; c += threads)
        *reinterpret_cast<uint4*>(job.dst + head + 16ull * c) = *reinterpret_cast<const uint4*>(src + head + 16ull * c);
    const uint32_t t = head + 16u * chunks + tid;
    if (t < n) job.dst[t] = src[t];
    if (tid == 0) final_len[job.slot] = n;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------

int64_t lz4_bound(int64_t n) { return n < 0 || n > (int64_t)kLzMaxInput ? 0 : n + n / 255 + 16; }             // LZ4_COMPRESSBOUND

// 1 and 2 channels are QOI-Plane and exist while the codec's switch is on (gamut_hip_qoix_set_plane)
bool desc_ok(const gamut_hip_qoix_desc& d)
{
    const bool channels_ok = (d.channels >= 3 && d.channels <= 4) || ((d.channels == 1 || d.channels == 2) && qoix_plane_on());
    return d.width > 0 && d.height > 0 && channels_ok && d.colorspace >= 0 && d.colorspace <= 2 &&
           (d.mode == 0 || d.mode == 1) && (uint32_t)d.height < kPixelsMax / (uint32_t)d.width;
}

// the most bytes the stored stream behind the header can have: colour, a pixel's channels + 1 and the four closing bytes; grey, 3 or
// 6 nibbles a pixel, the closing nine and one more to end on a byte (DEVIATION G1)
int64_t datalen_max_of(const gamut_hip_qoix_desc& d)
{
    const int64_t px = (int64_t)d.width * d.height;
    return d.channels >= 3 ? px * (d.channels + 1) + 4 : (px * (d.channels == 1 ? 3 : 6) + 10) / 2;
}

int64_t encode_bound(const gamut_hip_qoix_desc* d)
{
    if (!d || !desc_ok(*d)) return -1;
    if (d->channels == 2 && (int64_t)d->width * d->height * 6 > 0x7fffffffLL) return -1;      // DEVIATION G2
    const int64_t datalen_max = datalen_max_of(*d);
    const int64_t b = kHeader + 4 + datalen_max + datalen_max / 255 + 16;
    return b > 0x7fffffffLL ? -1 : b;                                        // DEVIATION 2
}

uint32_t float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// Measurements (tools/qoix_encode_bench.py): with GAMUT_HIP_QOIX_TIMING=1 the encode call brackets its three launches with events and
// keeps the GPU times of the calling thread's last call.
thread_local float t_last_encode_stage_ms[3] = { -1.0f, -1.0f, -1.0f };
thread_local float t_last_plane_stage_ms[3] = { -1.0f, -1.0f, -1.0f };       // k_qpenc_count, k_qpenc_scan, k_qpenc_write

int encode_batch(const uint8_t* const* src, const int64_t* src_pitch, const gamut_hip_qoix_desc* descs, int count, const int64_t* out_offset,
                 uint8_t* out, int64_t* out_len, int* status_host, hipStream_t stream)
{
    std::vector<QeImg> imgs; std::vector<LzJob> lzs; std::vector<PickJob> picks; std::vector<int> which; std::vector<size_t> at_stored, at_cand;
    int first_bad = -1;
    size_t scratch = 0;
    for (int i = 0; i < count; ++i) {
        out_len[i] = 0;
        const bool ok = encode_bound(&descs[i]) > 0 && src[i] && out_offset[i] >= 0;
        if (status_host) status_host[i] = ok ? GAMUT_HIP_OK : GAMUT_HIP_ERR_INVALID_ARG;
        if (!ok) { if (first_bad < 0) first_bad = i; continue; }
        const gamut_hip_qoix_desc& d = descs[i];
        QeImg im{};
        im.src = src[i]; im.pitch = src_pitch[i]; im.dst = out + out_offset[i];
        im.w = (uint32_t)d.width; im.h = (uint32_t)d.height; im.par = float_bits(d.pixel_aspect_ratio); im.dpi = float_bits(d.resolution_y);
        im.ch = (uint8_t)d.channels; im.cs = (uint8_t)d.colorspace;
        im.slot = (uint32_t)imgs.size();
        size_t a = (size_t)-1, c = (size_t)-1;
        if (d.mode == 0) {                                                   // both candidates in scratch, congruent to the destination modulo 16
            const size_t datalen_max = (size_t)datalen_max_of(d), shift = (uintptr_t)im.dst & 15u;
            a = scratch + shift; scratch += up16(shift + kHeader + datalen_max) + 16;
            c = scratch + shift; scratch += up16(shift + kHeader + 4 + (size_t)lz4_bound((int64_t)datalen_max)) + 16;
        }
        at_stored.push_back(a); at_cand.push_back(c);
        imgs.push_back(im); which.push_back(i);
    }
    if (!imgs.empty()) {
        const size_t n = imgs.size();
        size_t nlz = 0;
        for (size_t k = 0; k < n; ++k) nlz += at_stored[k] != (size_t)-1;
        size_t ngrey = 0, nsegs = 0;
        for (size_t k = 0; k < n; ++k)
            if (imgs[k].ch < 3) { ++ngrey; nsegs += ((size_t)imgs[k].w * imgs[k].h + kSeg - 1) / kSeg; }
        if (nsegs > 0x7fffffffu) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "qoix_encode: %zu segments of grey images in one call", nsegs);
        const size_t ncol = n - ngrey;
        const size_t o_img = 0, o_grey = up256(ncol * sizeof(QeImg) + 4), o_lz = o_grey + up256(ngrey * sizeof(QpImg) + 4),
                     o_pick = o_lz + up256(nlz * sizeof(LzJob) + 4), o_len = o_pick + up256(nlz * sizeof(PickJob) + 4),
                     staged = o_len, o_lzlen = o_len + up256(n * 4), o_fin = o_lzlen + up256(n * 4), lens_end = o_fin + up256(n * 4),
                     o_seg = lens_end, o_place = o_seg + up256(nsegs * sizeof(QpSeg)), o_scratch = o_place + up256(nsegs * sizeof(QpPlace)),
                     total = o_scratch + scratch;
        static thread_local PerDevice<DeviceScratch> scratch_pd;
        static thread_local PerDevice<PinnedScratch> pinned_pd;
        uint8_t* d = (uint8_t*)scratch_pd.cur().get(total, stream);
        uint8_t* h = pinned_pd.cur().get(lens_end, stream);
        if (!d || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "qoix_encode: scratch allocation of %zu bytes failed", total);
        for (size_t k = 0; k < n; ++k) {
            if (at_stored[k] == (size_t)-1) continue;
            uint8_t* stored = d + o_scratch + at_stored[k];
            uint8_t* cand = d + o_scratch + at_cand[k];
            lzs.push_back(LzJob{ stored, cand, 0u, 1u, imgs[k].slot, 0u });
            picks.push_back(PickJob{ stored, cand, imgs[k].dst, imgs[k].slot, 0u });
            imgs[k].dst = stored;
        }
        memset(h, 0, staged);
        QeImg* colour = (QeImg*)(h + o_img); QpImg* grey = (QpImg*)(h + o_grey);
        uint32_t seg0 = 0;
        for (size_t k = 0; k < n; ++k) {
            if (imgs[k].ch >= 3) { *colour++ = imgs[k]; continue; }
            const uint32_t nseg = (uint32_t)(((size_t)imgs[k].w * imgs[k].h + kSeg - 1) / kSeg);
            *grey++ = QpImg{ imgs[k], seg0, nseg };
            seg0 += nseg;
        }
        if (nlz) { memcpy(h + o_lz, lzs.data(), nlz * sizeof(LzJob)); memcpy(h + o_pick, picks.data(), nlz * sizeof(PickJob)); }
        GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, staged, hipMemcpyHostToDevice, stream));
        uint32_t* d_len = (uint32_t*)(d + o_len); uint32_t* d_lz = (uint32_t*)(d + o_lzlen); uint32_t* d_fin = (uint32_t*)(d + o_fin);
        static const bool timing = env_flag("GAMUT_HIP_QOIX_TIMING");
        KernelTimer<7> timer(timing);
        timer.mark(stream);
        if (ncol) hipLaunchKernelGGL(k_qxenc_ops, dim3((uint32_t)ncol), dim3(kWave), 0, stream, (const QeImg*)(d + o_img), d_len);
        timer.mark(stream);
        if (ngrey) {                                                         // three launches whatever the grey images are
            const QpImg* d_grey = (const QpImg*)(d + o_grey);
            hipLaunchKernelGGL(k_qpenc_count, dim3((uint32_t)nsegs), dim3(kWave), 0, stream, d_grey, (int)ngrey, (QpSeg*)(d + o_seg));
            timer.mark(stream);
            hipLaunchKernelGGL(k_qpenc_scan, dim3((uint32_t)ngrey), dim3(kWave), 0, stream, d_grey, (const QpSeg*)(d + o_seg), (QpPlace*)(d + o_place), d_len);
            timer.mark(stream);
            hipLaunchKernelGGL(k_qpenc_write, dim3((uint32_t)nsegs), dim3(kWave), 0, stream, d_grey, (int)ngrey, (const QpPlace*)(d + o_place));
        } else { timer.mark(stream); timer.mark(stream); }
        timer.mark(stream);
        hipLaunchKernelGGL(k_qxenc_lz4, dim3((uint32_t)std::max<size_t>(nlz, 1)), dim3(kWave), 0, stream, (const LzJob*)(d + o_lz), (int)nlz,
                           (const uint32_t*)d_len, d_lz);
        timer.mark(stream);
        hipLaunchKernelGGL(k_qxenc_pick, dim3((uint32_t)std::max<size_t>(nlz, 1), kPickBlocks), dim3(kPickThreads), 0, stream,
                           (const PickJob*)(d + o_pick), (int)nlz, (const uint32_t*)d_len, (const uint32_t*)d_lz, d_fin);
        if (int rc = launch_status("qoix_encode")) return rc;
        timer.mark(stream);
        GAMUT_HIP_CHECK(hipMemcpyAsync(h + o_len, d + o_len, lens_end - o_len, hipMemcpyDeviceToHost, stream));
        GAMUT_HIP_CHECK(hipStreamSynchronize(stream));
        if (timing) {
            float ms[6];
            timer.finish(ms);
            t_last_encode_stage_ms[0] = ms[0]; t_last_encode_stage_ms[1] = ms[4]; t_last_encode_stage_ms[2] = ms[5];
            for (int k = 0; k < 3; ++k) t_last_plane_stage_ms[k] = ngrey ? ms[1 + k] : -1.0f;
        }
        const uint32_t* stored_len = (const uint32_t*)(h + o_len); const uint32_t* fin = (const uint32_t*)(h + o_fin);
        for (size_t k = 0; k < n; ++k) out_len[which[k]] = at_stored[k] == (size_t)-1 ? stored_len[k] : fin[k];
    }
    if (first_bad >= 0) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "image %d: qoix_encode: refused description or source", first_bad);
    return GAMUT_HIP_OK;
}

int lz4_batch(const uint8_t* const* src, const int32_t* len, int count, const int64_t* out_offset, uint8_t* out, int64_t* out_len,
              int* status_host, hipStream_t stream)
{
    std::vector<LzJob> jobs; std::vector<int> which;
    int first_bad = -1;
    for (int i = 0; i < count; ++i) {
        out_len[i] = 0;
        const bool ok = src[i] && len[i] >= 0 && (uint32_t)len[i] <= kLzMaxInput && out_offset[i] >= 0;
        if (status_host) status_host[i] = ok ? GAMUT_HIP_OK : GAMUT_HIP_ERR_INVALID_ARG;
        if (!ok) { if (first_bad < 0) first_bad = i; continue; }
        jobs.push_back(LzJob{ src[i], out + out_offset[i], (uint32_t)len[i], 0u, (uint32_t)jobs.size(), 0u });
        which.push_back(i);
    }
    if (!jobs.empty()) {
        const size_t n = jobs.size(), o_len = up256(n * sizeof(LzJob)), total = o_len + up256(n * 4);
        static thread_local PerDevice<DeviceScratch> scratch_pd;
        static thread_local PerDevice<PinnedScratch> pinned_pd;
        uint8_t* d = (uint8_t*)scratch_pd.cur().get(total, stream);
        uint8_t* h = pinned_pd.cur().get(total, stream);
        if (!d || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "lz4_compress: scratch allocation of %zu bytes failed", total);
        memcpy(h, jobs.data(), n * sizeof(LzJob));
        GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, n * sizeof(LzJob), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_qxenc_lz4, dim3((uint32_t)n), dim3(kWave), 0, stream, (const LzJob*)d, (int)n, (const uint32_t*)nullptr, (uint32_t*)(d + o_len));
        if (int rc = launch_status("lz4_compress")) return rc;
        GAMUT_HIP_CHECK(hipMemcpyAsync(h + o_len, d + o_len, n * 4, hipMemcpyDeviceToHost, stream));
        GAMUT_HIP_CHECK(hipStreamSynchronize(stream));
        const uint32_t* lens = (const uint32_t*)(h + o_len);
        for (size_t k = 0; k < n; ++k) out_len[which[k]] = lens[k];
    }
    if (first_bad >= 0) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "image %d: lz4_compress: refused source, length or offset", first_bad);
    return GAMUT_HIP_OK;
}

} // namespace
} // namespace gamut

using namespace gamut;

extern "C" {

int64_t gamut_hip_qoix_encode_bound(const gamut_hip_qoix_desc* desc) { return encode_bound(desc); }

int gamut_hip_qoix_encode_window(void) { return kWave; }

int gamut_hip_qoix_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const gamut_hip_qoix_desc* descs, int count,
                                       const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!src || !src_pitch || !descs || !out_offset || !out || !out_len)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "qoix_encode_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return encode_batch(src, src_pitch, descs, count, out_offset, out, out_len, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "qoix_encode_batch_device: out of host memory");
    }
}

void* gamut_hip_qoix_write_to_mem(const void* data, int pitch, const gamut_hip_qoix_desc* desc, int* out_len)
{
    clear_error();
    if (!data || !out_len || encode_bound(desc) < 0) {
        set_error(GAMUT_HIP_ERR_INVALID_ARG, "qoix_write_to_mem: invalid arguments"); return nullptr;
    }
    if (!have_device()) return nullptr;
    const gamut_hip_qoix_desc d = *desc;
    return encode_host_image("qoix_write_to_mem", HostRows{ data, pitch, (size_t)d.width * d.channels, d.height, 1, 0 }, (size_t)encode_bound(&d), out_len,
        [&](const uint8_t* src, int64_t spitch, int64_t, int64_t off, uint8_t* dev, int64_t* n, hipStream_t st) {
            int status = 0;
            return encode_batch(&src, &spitch, &d, 1, &off, dev, n, &status, st);
        });
}

int gamut_hip_lz4_compress_bound(int n) { return (int)lz4_bound(n); }

int gamut_hip_lz4_compress_batch_device(const uint8_t* const* src, const int32_t* len, int count, const int64_t* out_offset, uint8_t* out,
                                        int64_t* out_len, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!src || !len || !out_offset || !out || !out_len)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "lz4_compress_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return lz4_batch(src, len, count, out_offset, out, out_len, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "lz4_compress_batch_device: out of host memory");
    }
}

float gamut_hip_qoix_last_encode_kernel_ms(void)
{
    const float* t = t_last_encode_stage_ms;
    return t[0] < 0 || t[1] < 0 || t[2] < 0 ? -1.0f : t[0] + t[1] + t[2];
}

float gamut_hip_qoix_last_encode_stage_ms(int stage) { return stage >= 0 && stage < 3 ? t_last_encode_stage_ms[stage] : -1.0f; }

int gamut_hip_qoix_plane_encode_segment(void) { return (int)kSeg; }

float gamut_hip_qoix_last_plane_encode_stage_ms(int stage) { return stage >= 0 && stage < 3 ? t_last_plane_stage_ms[stage] : -1.0f; }

} // extern "C"
