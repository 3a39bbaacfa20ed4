// png_encode.hip -- PNG encode on the GPU: the container and the filtered bytes of stbi_write_png_to_mem
// (codecs/stb_image_write.d:254-451) around a DEFLATE stream of our own, many images per batch.
//
// The reference hands its filtered rows to miniz; any valid zlib stream serves a reader, so the compressor here is built for
// the GPU: the filtered stream of an image is cut into blocks of kBlock bytes that are compressed independently (a block may
// match back into the 32 KiB before it: the whole filtered stream is in memory before the parse starts).  Five plain launches
// per chunk of images, no workgroup ever waits for another:
//   1. k_penc_filter : one workgroup per row: the five candidates' estimates, the choice, the type byte and the filtered row.
//   2. k_penc_block  : one workgroup per block: Adler-32 partials; a match per position (candidates: the distances filtered PNG
//                      data repeats at, lengths by dword compare); the greedy left-to-right parse (per-segment exit table, one
//                      short walk over the segments); histograms; length-limited Huffman code lengths (15 / 15 / 7 bits), the
//                      HLIT / HDIST / HCLEN header with its run-length coding; the smallest of stored / fixed / dynamic; the
//                      block's bits, starting at bit 0 of a scratch slot of its own.
//   3. k_penc_scan   : one lane per image: bit offsets of the blocks (a stored block's padding depends on where it starts),
//                      the total, the Adler-32 from the partials.
//   4. k_penc_place  : one workgroup per block: every payload byte is written once, by the block that holds its first bit (the
//                      bits a byte takes from the next block come from that block's first word): no atomics, no cleared words.
//   5. k_penc_finish : one workgroup per image: zlib header, Adler-32, signature, IHDR, IDAT length and CRC-32 (per-thread
//                      pieces combined by multiplication with x^(8 len) mod P), IEND, out_len.
// Stages 2-5 know nothing of PNG beyond the list of candidate distances in the image record.
#include "encode_host.hpp"
#include "device_util.hpp"
#include <climits>

namespace gamut {
namespace {

constexpr uint32_t kBlock = 8192;                     // filtered bytes per DEFLATE block
constexpr int kThreads = 256;
constexpr uint32_t kSeg = kBlock / kThreads;          // positions per thread in the parse (32)
constexpr uint32_t kSlotWords = kBlock / 4 + 4;       // scratch words per block: a compressed block has at most 8 n + 38 bits
constexpr uint32_t kMaxCand = 12;
constexpr uint32_t kMinMatch = 3, kMaxMatch = 258, kWindow = 32768;
constexpr uint32_t kNearDist = 8, kFarMinMatch = 6;  // matches of 3..5 are taken within 8 bytes only: further away they cost more bits than
                                                      // the literals they replace on filtered photographic data (measured)
constexpr uint64_t kChunkBytes = 512ull << 20;        // filtered bytes per launch set
constexpr size_t kChunkImages = 16384;
constexpr uint32_t kAdlerMod = 65521u, kCrcPoly = 0xEDB88320u;
constexpr int kContainer = 57;                        // signature 8 + IHDR 25 + IDAT 12 + IEND 12
constexpr int kPayloadAt = 41;                        // first payload byte: after the signature, IHDR, the IDAT length and tag

struct PImg {
    const uint8_t* src; int64_t pitch; int64_t out_off; uint64_t filt0;      // filt0: the image's first byte in the chunk's filtered scratch
    uint32_t w, h, n, is16, lb, L, row0, blk0, nblk, ncand;                  // lb = lineBytes; L = (lb + 1) * h
    int32_t force, level;
    uint32_t cand[kMaxCand];                                                 // ascending, distinct, 1..32768
};
struct PBlk { uint32_t bits, kind, s1, s2; };         // kind 0 stored, 1 compressed; s1 / s2: Adler partials of the block's bytes

__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) { for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64); return v; }
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) { for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64); return v; }

// ---- 1. filter ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ppaeth(int a, int b, int c)            // stbiw__paeth, :262-268
{
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    if (pa <= pb && pa <= pc) return a;
    if (pb <= pc) return b;
    return c;
}
// output byte p of row y under filter `type`.  The reference predicts on the native bytes and swaps the pairs of a 16-bit row
// afterwards (:336-351), so output byte p is the prediction of native byte p ^ 1.  Row 0 goes through firstmap (:279): no row above
// is the same arithmetic with b = c = 0; the first pixel (:316-326) is the same arithmetic with a = c = 0.
__device__ __forceinline__ uint8_t pfilt(const uint8_t* z, int64_t pitch, bool top, uint32_t bps, uint32_t is16, uint32_t p, int type)
{
    const uint32_t i = is16 ? p ^ 1u : p;
    const int v = z[i];
    if (type == 0) return (uint8_t)v;
    const bool left = i >= bps;
    const int a = left ? z[i - bps] : 0;
    if (type == 1) return (uint8_t)(v - a);
    const int b = top ? 0 : (z - pitch)[i];
    if (type == 2) return (uint8_t)(v - b);
    if (type == 3) return (uint8_t)(v - ((a + b) >> 1));
    const int c = (top || !left) ? 0 : (z - pitch)[i - bps];
    return (uint8_t)(v - ppaeth(a, b, c));
}

__global__ __launch_bounds__(kThreads) void k_penc_filter(const PImg* imgs, int n_img, uint32_t n_rows, uint8_t* filt)
{
    __shared__ uint32_t part[kThreads / 64][5];
    __shared__ int chosen;
    const int t = threadIdx.x;
    for (uint32_t g = blockIdx.x; g < n_rows; g += gridDim.x) {
        const PImg& im = imgs[find_unit<&PImg::row0>(imgs, n_img, g)];
        const uint32_t y = g - im.row0, bps = im.n * (im.is16 ? 2u : 1u), est_n = im.w * im.n;
        const uint8_t* z = im.src + (int64_t)y * im.pitch;
        const bool top = y == 0;
        int type = im.force;
        if (type < 0) {                                                // estimate over the first x * n bytes of each candidate (:394)
            uint32_t e[5] = { 0, 0, 0, 0, 0 };
            for (uint32_t p = t; p < est_n; p += kThreads) {
                #pragma unroll
                for (int k = 0; k < 5; ++k) e[k] += (uint32_t)abs((int)(int8_t)pfilt(z, im.pitch, top, bps, im.is16, p, k));
            }
            #pragma unroll
            for (int k = 0; k < 5; ++k) { e[k] = wave_sum32(e[k]); if ((t & 63) == 0) part[t >> 6][k] = e[k]; }
            __syncthreads();
            if (t == 0) {
                int best = 0; uint32_t best_val = 0x7fffffffu;
                for (int k = 0; k < 5; ++k) {
                    uint32_t s = 0;
                    for (int wv = 0; wv < kThreads / 64; ++wv) s += part[wv][k];
                    if (s < best_val) { best_val = s; best = k; }      // the first strictly smaller estimate wins (:397)
                }
                chosen = best;
            }
            __syncthreads();
            type = chosen;
        }
        uint8_t* o = filt + im.filt0 + (uint64_t)y * (im.lb + 1);
        if (t == 0) o[0] = (uint8_t)type;
        for (uint32_t p = t; p < im.lb; p += kThreads) o[1 + p] = pfilt(z, im.pitch, top, bps, im.is16, p, type);
        __syncthreads();                                               // part / chosen are reused by the next row
    }
}

// ---- 2. one DEFLATE block ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t match_len(const uint8_t* a, uint32_t d, uint32_t maxlen)
{
    const uint8_t* b = a - d;
    uint32_t l = 0;
    while (l + 4 <= maxlen) {
        uint32_t x, y;
        __builtin_memcpy(&x, a + l, 4); __builtin_memcpy(&y, b + l, 4);
        const uint32_t zz = x ^ y;
        if (zz) return l + ((uint32_t)__ffs((int)zz) - 1u) / 8u;
        l += 4;
    }
    while (l < maxlen && a[l] == b[l]) ++l;
    return l;
}
// length 3..258 -> code 0..28 (symbol 257 + code), extra bit count and value (RFC 1951 3.2.5)
__device__ __forceinline__ void len_code(uint32_t l, uint32_t& code, uint32_t& eb, uint32_t& ev)
{
    if (l == 258) { code = 28; eb = 0; ev = 0; return; }
    const uint32_t v = l - 3;
    if (v < 8) { code = v; eb = 0; ev = 0; return; }
    eb = (31u - (uint32_t)__clz((int)v)) - 2u;
    code = 4u + 4u * eb + ((v >> eb) & 3u);
    ev = v & ((1u << eb) - 1u);
}
// distance 1..32768 -> code 0..29
__device__ __forceinline__ void dist_code(uint32_t d, uint32_t& code, uint32_t& eb, uint32_t& ev)
{
    const uint32_t v = d - 1;
    if (v < 4) { code = v; eb = 0; ev = 0; return; }
    eb = (31u - (uint32_t)__clz((int)v)) - 1u;
    code = 2u + 2u * eb + ((v >> eb) & 1u);
    ev = v & ((1u << eb) - 1u);
}
__device__ __forceinline__ uint32_t fixed_ll_len(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }

// Huffman workspace of one tree inside the shared region (words)
constexpr uint32_t kWsSorted = 0, kWsFreq = 144, kWsParent = 144 + 576, kWsDepth = 144 + 576 + 288, kWsCount = 144 + 576 + 288 + 288,
                   kWsWords = 144 + 576 + 288 + 288 + 32;             // kWsCount: 16 counts + 16 next codes

// all threads: the symbols with a non-zero count, ascending by (count, symbol), into sorted[]; *m = how many.  *m must be 0 on entry.
__device__ __forceinline__ void huff_rank_sort(const uint32_t* freq, uint32_t nsym, uint32_t* ws, uint32_t* m, int t)
{
    uint16_t* sorted = reinterpret_cast<uint16_t*>(ws + kWsSorted);
    for (uint32_t s = t; s < nsym; s += kThreads) {
        const uint32_t f = freq[s];
        if (!f) continue;
        uint32_t r = 0;
        for (uint32_t u = 0; u < nsym; ++u) { const uint32_t fu = freq[u]; r += (fu && (fu < f || (fu == f && u < s))) ? 1u : 0u; }
        sorted[r] = (uint16_t)s;
        atomicAdd(m, 1u);
    }
}
// one lane: code lengths of at most maxbits from the sorted symbols (two-queue Huffman merge, depths clamped, Kraft sum repaired by
// moving one leaf down per unit of excess, lengths handed out longest first to the rarest symbols)
__device__ void huff_build(const uint32_t* freq, uint32_t nsym, uint32_t m, uint32_t maxbits, uint8_t* lens, uint32_t* ws)
{
    const uint16_t* sorted = reinterpret_cast<const uint16_t*>(ws + kWsSorted);
    uint32_t* nf = ws + kWsFreq;
    uint16_t* parent = reinterpret_cast<uint16_t*>(ws + kWsParent);
    uint16_t* depth = reinterpret_cast<uint16_t*>(ws + kWsDepth);
    uint32_t* count = ws + kWsCount;
    for (uint32_t s = 0; s < nsym; ++s) lens[s] = 0;
    if (m == 0) return;
    if (m == 1) { lens[sorted[0]] = 1; return; }
    for (uint32_t i = 0; i < m; ++i) nf[i] = freq[sorted[i]];
    uint32_t li = 0, ii = m, next = m;
    for (uint32_t k = 0; k + 1 < m; ++k) {
        uint32_t a, b;
        if (li < m && (ii >= next || nf[li] <= nf[ii])) a = li++; else a = ii++;
        if (li < m && (ii >= next || nf[li] <= nf[ii])) b = li++; else b = ii++;
        nf[next] = nf[a] + nf[b];
        parent[a] = (uint16_t)next; parent[b] = (uint16_t)next;
        ++next;
    }
    const uint32_t root = 2 * m - 2;
    depth[root] = 0;
    for (int k = (int)root - 1; k >= 0; --k) depth[k] = (uint16_t)(depth[parent[k]] + 1);
    for (uint32_t l = 0; l <= maxbits; ++l) count[l] = 0;
    for (uint32_t i = 0; i < m; ++i) { const uint32_t d = depth[i] < maxbits ? depth[i] : maxbits; count[d] += 1; }
    uint32_t total = 0;
    for (uint32_t l = 1; l <= maxbits; ++l) total += count[l] << (maxbits - l);
    while (total > (1u << maxbits)) {
        count[maxbits] -= 1;
        for (uint32_t l = maxbits - 1; l >= 1; --l)
            if (count[l]) { count[l] -= 1; count[l + 1] += 2; break; }
        total -= 1;
    }
    uint32_t i = 0;
    for (uint32_t l = maxbits; l >= 1; --l)
        for (uint32_t c = count[l]; c > 0; --c) lens[sorted[i++]] = (uint8_t)l;
}
// one lane: canonical codes from lengths, bit-reversed for the LSB-first stream
__device__ void huff_codes(const uint8_t* lens, uint32_t nsym, uint16_t* codes, uint32_t* ws)
{
    uint32_t* count = ws;            // 16 counts, then 16 next codes
    uint32_t* nextc = ws + 16;
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (uint32_t s = 0; s < nsym; ++s) count[lens[s]] += 1;
    count[0] = 0;
    uint32_t code = 0;
    for (int l = 1; l < 16; ++l) { code = (code + count[l - 1]) << 1; nextc[l] = code; }
    for (uint32_t s = 0; s < nsym; ++s) {
        const uint32_t l = lens[s];
        if (!l) { codes[s] = 0; continue; }
        const uint32_t c = nextc[l]; nextc[l] = c + 1;
        codes[s] = (uint16_t)(__brev(c) >> (32 - l));
    }
}
__device__ __forceinline__ void put_bits(uint32_t* buf, uint32_t pos, uint64_t v, uint32_t n)      // n <= 57, bits above n are zero
{
    const uint32_t w = pos >> 5, s = pos & 31u;
    const uint64_t x = v << s;                                         // s + n <= 88: the part above bit 63 goes to the third word
    const uint32_t lo = (uint32_t)x, mid = (uint32_t)(x >> 32);
    if (lo) atomicOr(&buf[w], lo);
    if (mid) atomicOr(&buf[w + 1], mid);
    if (s + n > 64) { const uint32_t hi = (uint32_t)(v >> (64 - s)); if (hi) atomicOr(&buf[w + 2], hi); }
}

__constant__ uint8_t c_clorder[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };

__global__ __launch_bounds__(kThreads) void k_penc_block(const PImg* imgs, int n_img, const uint8_t* filt, PBlk* meta, uint32_t* slots)
{
    __shared__ uint16_t mlen[kBlock], mdist[kBlock];
    __shared__ uint32_t region[kBlock / 2];            // exit table (u16 x kBlock), then Huffman workspaces, then the block's bits
    __shared__ uint16_t entry[kThreads];
    __shared__ uint32_t hist_ll[288], hist_d[32], hist_cl[19];
    __shared__ uint8_t len_ll[288], len_d[32], len_cl[19];
    __shared__ uint16_t code_ll[288], code_d[32], code_cl[19];
    __shared__ uint16_t rle[320];
    __shared__ uint32_t sh_m[2], sh_nrle, sh_hlit, sh_hdist, sh_hclen, sh_hdr, sh_kind;
    __shared__ uint64_t red[kThreads / 64][2];
    __shared__ uint32_t scan_part[kThreads / 64];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t g = blockIdx.x;
    const PImg& im = imgs[find_unit<&PImg::blk0>(imgs, n_img, g)];
    const uint32_t b = g - im.blk0, s0 = b * kBlock, n = min(kBlock, im.L - s0);
    const uint8_t* f = filt + im.filt0;                // the image's filtered stream; the block is f[s0, s0 + n)
    const uint8_t* blk = f + s0;
    const uint32_t a0 = t * kSeg, a1 = min(a0 + kSeg, n);
    const bool last = b + 1 == im.nblk;

    // Adler-32 partials: s1 = sum d_i, s2 = sum (n - i) d_i
    {
        uint32_t s1 = 0, s2 = 0;
        for (uint32_t i = a0; i < a1; ++i) { const uint32_t d = blk[i]; s1 += d; s2 += (n - i) * d; }
        uint64_t r1 = wave_sum64(s1), r2 = wave_sum64(s2);
        if (lane == 0) { red[wave][0] = r1; red[wave][1] = r2; }
        __syncthreads();
        if (t == 0) {
            r1 = 0; r2 = 0;
            for (int k = 0; k < kThreads / 64; ++k) { r1 += red[k][0]; r2 += red[k][1]; }
            meta[g].s1 = (uint32_t)(r1 % kAdlerMod); meta[g].s2 = (uint32_t)(r2 % kAdlerMod);
            if (im.level == 0) { meta[g].kind = 0; meta[g].bits = 0; }
        }
        __syncthreads();
    }
    if (im.level == 0) return;                          // stored blocks only

    // a match per position
    for (uint32_t i = t; i < n; i += kThreads) {
        const uint32_t p = s0 + i, maxlen = min(kMaxMatch, n - i);
        uint32_t best = 1, bd = 1;
        if (maxlen >= kMinMatch) {
            for (uint32_t c = 0; c < im.ncand; ++c) {
                const uint32_t d = im.cand[c];
                if (d > p) break;
                if (blk[i] != (blk + i - d)[0]) continue;
                const uint32_t l = match_len(blk + i, d, maxlen);
                if (l > best && (l >= kFarMinMatch || (l >= kMinMatch && d <= kNearDist))) { best = l; bd = d; if (l == maxlen) break; }
            }
        }
        mlen[i] = (uint16_t)best; mdist[i] = (uint16_t)(bd - 1);
    }
    __syncthreads();

    // greedy parse: exitp[i] = the first position at or past the segment's end that the walk from i reaches
    uint16_t* exitp = reinterpret_cast<uint16_t*>(region);
    for (int i = (int)a1 - 1; i >= (int)a0; --i) {
        const uint32_t nx = (uint32_t)i + mlen[i];
        exitp[i] = (uint16_t)(nx >= a1 ? nx : exitp[nx]);
    }
    entry[t] = 0xFFFFu;
    for (int k = t; k < 288; k += kThreads) hist_ll[k] = 0;
    if (t < 32) hist_d[t] = 0;
    if (t < 19) hist_cl[t] = 0;
    if (t < 2) sh_m[t] = 0;
    __syncthreads();
    if (t == 0) {
        for (uint32_t pos = 0; pos < n; pos = exitp[pos]) entry[pos / kSeg] = (uint16_t)pos;
        hist_ll[256] = 1;
    }
    __syncthreads();

    // histograms
    if (entry[t] != 0xFFFFu) {
        for (uint32_t pos = entry[t]; pos < a1; ) {
            const uint32_t l = mlen[pos];
            if (l == 1) atomicAdd(&hist_ll[blk[pos]], 1u);
            else {
                uint32_t c, eb, ev;
                len_code(l, c, eb, ev); atomicAdd(&hist_ll[257 + c], 1u);
                dist_code((uint32_t)mdist[pos] + 1u, c, eb, ev); atomicAdd(&hist_d[c], 1u);
            }
            pos += l;
        }
    }
    __syncthreads();
    if (t == 0) {                                       // a distance tree needs two codes to be complete
        if (!hist_d[0]) hist_d[0] = 1;
        uint32_t nz = 0;
        for (int k = 0; k < 30; ++k) nz += hist_d[k] ? 1u : 0u;
        if (nz < 2) hist_d[1] = 1;
    }
    __syncthreads();

    // code lengths: literal/length on lane 0 of wave 0, distance on lane 0 of wave 1
    uint32_t* ws0 = region, * ws1 = region + kWsWords;
    huff_rank_sort(hist_ll, 286, ws0, &sh_m[0], t);
    huff_rank_sort(hist_d, 30, ws1, &sh_m[1], t);
    __syncthreads();
    if (t == 0) { huff_build(hist_ll, 286, sh_m[0], 15, len_ll, ws0); len_ll[286] = 0; len_ll[287] = 0; huff_codes(len_ll, 286, code_ll, ws0 + kWsCount); }
    if (t == 64) { huff_build(hist_d, 30, sh_m[1], 15, len_d, ws1); len_d[30] = 0; len_d[31] = 0; huff_codes(len_d, 30, code_d, ws1 + kWsCount); }
    __syncthreads();

    // the code-length code: run-length tokens of the HLIT + HDIST lengths, their Huffman code (7 bits), the header's bit count
    if (t == 0) {
        uint32_t hlit = 286, hdist = 30;
        while (hlit > 257 && !len_ll[hlit - 1]) --hlit;
        while (hdist > 1 && !len_d[hdist - 1]) --hdist;
        const uint32_t N = hlit + hdist;
        auto seq = [&](uint32_t i) -> uint32_t { return i < hlit ? len_ll[i] : len_d[i - hlit]; };
        uint32_t nr = 0;
        auto tok = [&](uint32_t sym, uint32_t extra) { rle[nr++] = (uint16_t)(sym | extra << 5); hist_cl[sym] += 1; };
        for (uint32_t i = 0; i < N; ) {
            const uint32_t v = seq(i);
            uint32_t run = 1;
            while (i + run < N && seq(i + run) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) { const uint32_t r = run < 138 ? run : 138; tok(18, r - 11); run -= r; }
                if (run >= 3) { tok(17, run - 3); run = 0; }
                while (run) { tok(0, 0); --run; }
            } else {
                tok(v, 0); --run;
                while (run >= 3) { const uint32_t r = run < 6 ? run : 6; tok(16, r - 3); run -= r; }
                while (run) { tok(v, 0); --run; }
            }
        }
        uint32_t nz = 0;
        for (int k = 0; k < 19; ++k) nz += hist_cl[k] ? 1u : 0u;
        if (nz < 2) { if (!hist_cl[0]) hist_cl[0] = 1; else hist_cl[1] = 1; }
        // 19 symbols: sorted by insertion on this lane
        uint16_t* sorted = reinterpret_cast<uint16_t*>(ws0 + kWsSorted);
        uint32_t m = 0;
        for (uint32_t s = 0; s < 19; ++s) {
            if (!hist_cl[s]) continue;
            uint32_t k = m++;
            while (k > 0 && hist_cl[sorted[k - 1]] > hist_cl[s]) { sorted[k] = sorted[k - 1]; --k; }
            sorted[k] = (uint16_t)s;
        }
        huff_build(hist_cl, 19, m, 7, len_cl, ws0);
        huff_codes(len_cl, 19, code_cl, ws0 + kWsCount);
        uint32_t hclen = 19;
        while (hclen > 4 && !len_cl[c_clorder[hclen - 1]]) --hclen;
        uint32_t hdr = 3 + 5 + 5 + 4 + 3 * hclen;
        for (uint32_t k = 0; k < nr; ++k) {
            const uint32_t sym = rle[k] & 31u;
            hdr += len_cl[sym] + (sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u);
        }
        sh_nrle = nr; sh_hlit = hlit; sh_hdist = hdist; sh_hclen = hclen; sh_hdr = hdr;
    }
    __syncthreads();

    // the tokens' bits under the dynamic and the fixed code
    uint32_t dyn = 0, fix = 0;
    if (entry[t] != 0xFFFFu) {
        for (uint32_t pos = entry[t]; pos < a1; ) {
            const uint32_t l = mlen[pos];
            if (l == 1) { const uint32_t s = blk[pos]; dyn += len_ll[s]; fix += fixed_ll_len(s); }
            else {
                uint32_t c, eb, ev, c2, eb2, ev2;
                len_code(l, c, eb, ev); dist_code((uint32_t)mdist[pos] + 1u, c2, eb2, ev2);
                dyn += len_ll[257 + c] + eb + len_d[c2] + eb2;
                fix += fixed_ll_len(257 + c) + eb + 5u + eb2;
            }
            pos += l;
        }
    }
    {
        const uint64_t r1 = wave_sum64(dyn), r2 = wave_sum64(fix);
        if (lane == 0) { red[wave][0] = r1; red[wave][1] = r2; }
        __syncthreads();
        if (t == 0) {
            uint64_t d = 0, x = 0;
            for (int k = 0; k < kThreads / 64; ++k) { d += red[k][0]; x += red[k][1]; }
            d += sh_hdr + len_ll[256]; x += 3 + 7;
            // A stored block costs 8 n + 40 bits when it starts on a byte and up to 2 more when it does not, which only happens
            // right after a compressed block: a compressed block is taken only when it is 2 bits cheaper, so no stream is ever
            // longer than the all-stored stream of level 0.
            const uint64_t stored = 8ull * n + 40, comp = d < x ? d : x;
            sh_kind = comp + 2 > stored ? 0u : d <= x ? 1u : 2u;
            if (sh_kind == 2) {                          // the fixed code through the same tables
                for (uint32_t s = 0; s < 288; ++s) len_ll[s] = (uint8_t)fixed_ll_len(s);
                for (uint32_t s = 0; s < 32; ++s) len_d[s] = 5;
                huff_codes(len_ll, 288, code_ll, region + kWsCount);
                huff_codes(len_d, 32, code_d, region + kWsCount);
                sh_hdr = 3;
            }
            meta[g].kind = sh_kind ? 1u : 0u;
            meta[g].bits = sh_kind ? (uint32_t)comp : 0u;
        }
        __syncthreads();
    }
    const uint32_t kind = sh_kind;
    if (kind == 0) return;

    // bit offsets of the threads' token runs, the bits into the region, the region into the block's slot
    const uint32_t mine = kind == 1 ? dyn : fix;
    uint32_t incl = mine;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(incl, d, 64); if (lane >= d) incl += u; }
    if (lane == 63) scan_part[wave] = incl;
    for (uint32_t k = t; k < kBlock / 2; k += kThreads) region[k] = 0;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (int k = 0; k < kThreads / 64; ++k) { if (k < wave) before += scan_part[k]; total += scan_part[k]; }
    const uint32_t hdr = sh_hdr;
    if (t == 0) {
        uint32_t at = 0;
        put_bits(region, at, (last ? 1u : 0u) | (kind == 1 ? 2u : 1u) << 1, 3); at += 3;
        if (kind == 1) {
            put_bits(region, at, sh_hlit - 257, 5); at += 5;
            put_bits(region, at, sh_hdist - 1, 5); at += 5;
            put_bits(region, at, sh_hclen - 4, 4); at += 4;
            for (uint32_t k = 0; k < sh_hclen; ++k) { put_bits(region, at, len_cl[c_clorder[k]], 3); at += 3; }
            for (uint32_t k = 0; k < sh_nrle; ++k) {
                const uint32_t sym = rle[k] & 31u, extra = rle[k] >> 5;
                put_bits(region, at, code_cl[sym], len_cl[sym]); at += len_cl[sym];
                const uint32_t eb = sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u;
                if (eb) { put_bits(region, at, extra, eb); at += eb; }
            }
        }
        put_bits(region, hdr + total, code_ll[256], len_ll[256]);      // end of block
    }
    if (entry[t] != 0xFFFFu) {
        uint32_t at = hdr + before + incl - mine;
        for (uint32_t pos = entry[t]; pos < a1; ) {
            const uint32_t l = mlen[pos];
            if (l == 1) { const uint32_t s = blk[pos]; put_bits(region, at, code_ll[s], len_ll[s]); at += len_ll[s]; }
            else {
                uint32_t c, eb, ev, c2, eb2, ev2;
                len_code(l, c, eb, ev); dist_code((uint32_t)mdist[pos] + 1u, c2, eb2, ev2);
                uint64_t v = code_ll[257 + c]; uint32_t nb = len_ll[257 + c];
                v |= (uint64_t)ev << nb; nb += eb;
                v |= (uint64_t)code_d[c2] << nb; nb += len_d[c2];
                v |= (uint64_t)ev2 << nb; nb += eb2;
                put_bits(region, at, v, nb); at += nb;
            }
            pos += l;
        }
    }
    __syncthreads();
    const uint32_t bits = hdr + total + len_ll[256], words = (bits + 31) >> 5;
    uint32_t* slot = slots + (uint64_t)g * kSlotWords;
    for (uint32_t k = t; k < words; k += kThreads) slot[k] = region[k];
}

// ---- 3. per-image scan ------------------------------------------------------------------------------------------------------------
// Bit positions count from the first payload byte: the zlib header holds bits 0..15.
__global__ __launch_bounds__(64) void k_penc_scan(const PImg* imgs, int n_img, const PBlk* meta, uint64_t* off, uint64_t* size,
                                                  uint64_t* tbits, uint32_t* adler)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_img) return;
    const PImg& im = imgs[i];
    uint64_t o = 16, a = 1, b2 = 0;
    for (uint32_t b = 0; b < im.nblk; ++b) {
        const uint32_t g = im.blk0 + b, n = min(kBlock, im.L - b * kBlock);
        const PBlk m = meta[g];
        const uint64_t c = m.kind ? (uint64_t)m.bits : (((o + 3 + 7) & ~7ull) - o) + 32 + 8ull * n;
        off[g] = o; size[g] = c; o += c;
        b2 = (b2 + (uint64_t)n * a + m.s2) % kAdlerMod;
        a = (a + m.s1) % kAdlerMod;
    }
    tbits[i] = o;
    adler[i] = (uint32_t)(b2 << 16 | a);
}

// ---- 4. placement -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_penc_place(const PImg* imgs, int n_img, const uint8_t* filt, const PBlk* meta,
                                                         const uint32_t* slots, const uint64_t* off, const uint64_t* size, uint8_t* out)
{
    const int t = threadIdx.x;
    const uint32_t g = blockIdx.x;
    const PImg& im = imgs[find_unit<&PImg::blk0>(imgs, n_img, g)];
    const uint32_t b = g - im.blk0, s0 = b * kBlock, n = min(kBlock, im.L - s0);
    const bool last = b + 1 == im.nblk;
    const uint64_t o = off[g], c = size[g];
    uint8_t* pay = out + im.out_off + kPayloadAt;
    const uint64_t j0 = (o + 7) >> 3, j1 = (o + c + 7) >> 3;          // the bytes whose first bit lies in [o, o + c)
    if (meta[g].kind) {
        const uint32_t* slot = slots + (uint64_t)g * kSlotWords;
        uint32_t nextfirst = 0;                                        // the first bits of what follows: the next block's, or padding
        if (!last) nextfirst = meta[g + 1].kind ? slots[(uint64_t)(g + 1) * kSlotWords] & 255u : (b + 2 == im.nblk ? 1u : 0u);
        for (uint64_t j = j0 + t; j < j1; j += kThreads) {
            const uint64_t q = 8 * j - o;
            const uint32_t w = (uint32_t)(q >> 5), s = (uint32_t)q & 31u;
            uint32_t v = slot[w] >> s;
            if (s > 24) v |= slot[w + 1] << (32 - s);
            const uint64_t valid = c - q;
            if (valid < 8) v = (v & ((1u << valid) - 1u)) | nextfirst << valid;
            pay[j] = (uint8_t)v;
        }
    } else {
        const uint64_t a = (o + 3 + 7) >> 3;                           // LEN, NLEN, then the bytes
        const uint8_t* d = filt + im.filt0 + s0;
        for (uint64_t j = j0 + t; j < j1; j += kThreads) {
            uint32_t v;
            if (j < a) v = (8 * j == o && last) ? 1u : 0u;
            else {
                const uint64_t k = j - a;
                v = k == 0 ? n & 255u : k == 1 ? n >> 8 : k == 2 ? ~n & 255u : k == 3 ? (~n >> 8) & 255u : d[k - 4];
            }
            pay[j] = (uint8_t)v;
        }
    }
}

// ---- 5. finish --------------------------------------------------------------------------------------------------------------------
// CRC-32 (reflected, x^0 = bit 31).  a * b mod P, and x^(8 n) mod P
__device__ __forceinline__ uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
__device__ __forceinline__ uint32_t crc_xpow8(uint64_t n)
{
    uint32_t p = 0x80000000u, base = 0x00800000u;
    for (; n; n >>= 1) { if (n & 1) p = crc_mul(base, p); base = crc_mul(base, base); }
    return p;
}
__device__ __forceinline__ uint32_t crc_bytes(uint32_t crc, const uint8_t* p, int n)      // bitwise, for a few bytes
{
    for (int i = 0; i < n; ++i) {
        crc ^= p[i];
        for (int k = 0; k < 8; ++k) crc = (crc & 1u) ? (crc >> 1) ^ kCrcPoly : crc >> 1;
    }
    return crc;
}
__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

constexpr int kFinThreads = 1024;
__global__ __launch_bounds__(kFinThreads) void k_penc_finish(const PImg* imgs, const uint64_t* tbits, const uint32_t* adler, uint8_t* out,
                                                             int64_t* out_len)
{
    __shared__ uint32_t table[256];
    __shared__ uint32_t piece[kFinThreads];
    const int t = threadIdx.x;
    const PImg& im = imgs[blockIdx.x];
    uint8_t* o = out + im.out_off;
    uint8_t* pay = o + kPayloadAt;
    const uint64_t P = ((tbits[blockIdx.x] + 7) >> 3) + 4;            // zlib header + blocks + Adler-32
    if (t < 256) {
        uint32_t c = (uint32_t)t;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        table[t] = c;
    }
    if (t == 0) {
        const int lv = im.level;                                       // CMF 0x78; FLG: FLEVEL by level, FCHECK makes the pair a multiple of 31
        pay[0] = 0x78; pay[1] = lv <= 1 ? 0x01 : lv <= 5 ? 0x5E : lv == 6 ? 0x9C : 0xDA;
        put_be32(pay + P - 4, adler[blockIdx.x]);
    }
    __threadfence();
    __syncthreads();
    const uint64_t per = (P + kFinThreads - 1) / kFinThreads, p0 = min(P, (uint64_t)t * per), p1 = min(P, p0 + per);
    uint32_t crc = 0xFFFFFFFFu;
    for (uint64_t k = p0; k < p1; ++k) crc = table[(crc ^ pay[k]) & 255u] ^ (crc >> 8);
    piece[t] = ~crc;
    __syncthreads();
    if (t == 0) {
        const uint8_t sig[8] = { 137, 80, 78, 71, 13, 10, 26, 10 };
        const uint8_t ctype[5] = { 0, 0, 4, 2, 6 };
        for (int k = 0; k < 8; ++k) o[k] = sig[k];
        put_be32(o + 8, 13);
        o[12] = 'I'; o[13] = 'H'; o[14] = 'D'; o[15] = 'R';
        put_be32(o + 16, im.w); put_be32(o + 20, im.h);
        o[24] = im.is16 ? 16 : 8; o[25] = ctype[im.n]; o[26] = 0; o[27] = 0; o[28] = 0;
        put_be32(o + 29, ~crc_bytes(0xFFFFFFFFu, o + 12, 17));
        put_be32(o + 33, (uint32_t)P);
        o[37] = 'I'; o[38] = 'D'; o[39] = 'A'; o[40] = 'T';
        uint32_t acc = ~crc_bytes(0xFFFFFFFFu, o + 37, 4);
        const uint32_t xfull = crc_xpow8(per);
        for (int k = 0; k < kFinThreads; ++k) {
            const uint64_t q0 = min(P, (uint64_t)k * per), q1 = min(P, q0 + per);
            if (q1 == q0) break;
            acc = crc_mul(q1 - q0 == per ? xfull : crc_xpow8(q1 - q0), acc) ^ piece[k];
        }
        uint8_t* e = pay + P;
        put_be32(e, acc);
        put_be32(e + 4, 0);
        e[8] = 'I'; e[9] = 'E'; e[10] = 'N'; e[11] = 'D';
        put_be32(e + 12, 0xAE426082u);
        out_len[blockIdx.x] = (int64_t)(kContainer + P);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// (lineBytes + 1) * h must fit a positive int: the reference computes it in int (:363-372)
bool pvalid(int w, int h, int comp, int is16)
{
    if (w < 1 || h < 1 || comp < 1 || comp > 4) return false;
    const int64_t lb = (int64_t)w * comp * (is16 ? 2 : 1);
    return (lb + 1) * (int64_t)h <= (int64_t)INT_MAX;
}
int64_t pfiltered(int w, int h, int comp, int is16) { return ((int64_t)w * comp * (is16 ? 2 : 1) + 1) * (int64_t)h; }
int64_t pbound(int w, int h, int comp, int is16)
{
    if (!pvalid(w, h, comp, is16)) return 0;
    const int64_t L = pfiltered(w, h, comp, is16);
    return kContainer + 6 + L + 5 * ((L + kBlock - 1) / kBlock);
}

// the distances filtered PNG data repeats at: the pixel sizes and their doubles, the row above and its neighbours, two rows up
void pcandidates(PImg& im)
{
    const uint32_t bpp = im.n * (im.is16 ? 2u : 1u), stride = im.lb + 1;
    std::vector<uint32_t> c = { 1, 2, 3, 4, 6, 8, 2 * bpp, stride, stride + bpp, 2 * stride };
    if (stride > bpp) c.push_back(stride - bpp);
    std::sort(c.begin(), c.end());
    c.erase(std::unique(c.begin(), c.end()), c.end());
    im.ncand = 0;
    for (uint32_t d : c) if (d >= 1 && d <= kWindow && im.ncand < kMaxCand) im.cand[im.ncand++] = d;
}

int pencode_chunk(std::vector<PImg>& imgs, const std::vector<int>& which, int64_t* out_len, uint8_t* out, hipStream_t stream)
{
    const int n = (int)imgs.size();
    uint64_t rows = 0, blks = 0, fb = 0;
    for (PImg& im : imgs) {
        im.row0 = (uint32_t)rows; im.blk0 = (uint32_t)blks; im.filt0 = fb;
        rows += im.h; blks += im.nblk; fb += ((uint64_t)im.L + 15) & ~15ull;
    }
    const size_t o_img = 0, o_meta = up256((size_t)n * sizeof(PImg)), o_off = o_meta + up256(blks * sizeof(PBlk)), o_size = o_off + up256(blks * 8),
                 o_t = o_size + up256(blks * 8), o_ad = o_t + up256((size_t)n * 8), o_len = o_ad + up256((size_t)n * 4), o_slots = o_len + up256((size_t)n * 8),
                 o_filt = o_slots + up256(blks * kSlotWords * 4), total = o_filt + up256(fb + 16);
    const size_t h_up = o_meta;
    static thread_local PerDevice<DeviceScratch> scratch_pd;
    static thread_local PerDevice<PinnedScratch> pinned_pd;
    uint8_t* d = (uint8_t*)scratch_pd.cur().get(total, stream);
    uint8_t* h = pinned_pd.cur().get(h_up + (size_t)n * 8, stream);
    if (!d || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "png_encode: scratch allocation of %zu bytes failed", total);
    memcpy(h + o_img, imgs.data(), (size_t)n * sizeof(PImg));
    GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, (size_t)n * sizeof(PImg), hipMemcpyHostToDevice, stream));
    const PImg* dimg = (const PImg*)(d + o_img);
    PBlk* meta = (PBlk*)(d + o_meta); uint64_t* off = (uint64_t*)(d + o_off); uint64_t* size = (uint64_t*)(d + o_size);
    uint64_t* tb = (uint64_t*)(d + o_t); uint32_t* ad = (uint32_t*)(d + o_ad); int64_t* len = (int64_t*)(d + o_len);
    uint32_t* slots = (uint32_t*)(d + o_slots); uint8_t* filt = d + o_filt;
    const uint32_t R = (uint32_t)rows, NB = (uint32_t)blks;
    hipLaunchKernelGGL(k_penc_filter, dim3(std::min(R, 1u << 20)), dim3(kThreads), 0, stream, dimg, n, R, filt);
    hipLaunchKernelGGL(k_penc_block, dim3(NB), dim3(kThreads), 0, stream, dimg, n, (const uint8_t*)filt, meta, slots);
    hipLaunchKernelGGL(k_penc_scan, dim3((n + 63) / 64), dim3(64), 0, stream, dimg, n, (const PBlk*)meta, off, size, tb, ad);
    hipLaunchKernelGGL(k_penc_place, dim3(NB), dim3(kThreads), 0, stream, dimg, n, (const uint8_t*)filt, (const PBlk*)meta,
                       (const uint32_t*)slots, (const uint64_t*)off, (const uint64_t*)size, out);
    hipLaunchKernelGGL(k_penc_finish, dim3(n), dim3(kFinThreads), 0, stream, dimg, (const uint64_t*)tb, (const uint32_t*)ad, out, len);
    if (int rc = launch_status("png_encode")) return rc;
    int64_t* hlen = (int64_t*)(h + h_up);
    GAMUT_HIP_CHECK(hipMemcpyAsync(hlen, len, (size_t)n * 8, hipMemcpyDeviceToHost, stream));
    GAMUT_HIP_CHECK(hipStreamSynchronize(stream));
    for (int k = 0; k < n; ++k) out_len[which[(size_t)k]] = hlen[k];
    return GAMUT_HIP_OK;
}

int pencode_batch(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width, const int32_t* height, const int32_t* comp,
                  const int32_t* is16bit, const int32_t* force_filter, const int32_t* level, int count, const int64_t* out_offset,
                  uint8_t* out, int64_t* out_len, int* status_host, hipStream_t stream)
{
    std::vector<PImg> imgs; std::vector<int> which;
    int first_bad = -1;
    for (int i = 0; i < count; ++i) {
        out_len[i] = 0;
        const int lv = level ? level[i] : 5, is16 = is16bit[i] ? 1 : 0;
        const bool ok = pvalid(width[i], height[i], comp[i], is16) && lv >= 0 && lv <= 10 && src[i] && out_offset[i] >= 0;
        if (status_host) status_host[i] = ok ? GAMUT_HIP_OK : GAMUT_HIP_ERR_INVALID_ARG;
        if (!ok) { if (first_bad < 0) first_bad = i; continue; }
        PImg im{};
        im.src = src[i]; im.pitch = src_pitch[i]; im.out_off = out_offset[i];
        im.w = (uint32_t)width[i]; im.h = (uint32_t)height[i]; im.n = (uint32_t)comp[i]; im.is16 = (uint32_t)is16;
        im.lb = im.w * im.n * (is16 ? 2u : 1u);
        im.L = (uint32_t)pfiltered(width[i], height[i], comp[i], is16);
        im.nblk = (im.L + kBlock - 1) / kBlock;
        const int ff = force_filter ? force_filter[i] : -1;
        im.force = (ff < 0 || ff >= 5) ? -1 : ff;                     // :365: 0..4 forces, everything else selects
        im.level = lv;
        pcandidates(im);
        imgs.push_back(im); which.push_back(i);
    }
    size_t a = 0;
    while (a < imgs.size()) {
        size_t b = a; uint64_t bytes = 0;
        while (b < imgs.size() && b - a < kChunkImages && (b == a || bytes + imgs[b].L <= kChunkBytes)) bytes += imgs[b++].L;
        std::vector<PImg> part(imgs.begin() + a, imgs.begin() + b);
        std::vector<int> w(which.begin() + a, which.begin() + b);
        if (int rc = pencode_chunk(part, w, out_len, out, stream)) return rc;
        a = b;
    }
    if (first_bad >= 0) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "image %d: png_encode: invalid size, comp, level or source", first_bad);
    return GAMUT_HIP_OK;
}

} // namespace
} // namespace gamut

using namespace gamut;

extern "C" {

int64_t gamut_hip_png_encode_bound(int width, int height, int comp, int is16bit) { return pbound(width, height, comp, is16bit ? 1 : 0); }

int gamut_hip_png_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width, const int32_t* height,
                                      const int32_t* comp, const int32_t* is16bit, const int32_t* force_filter, const int32_t* level,
                                      int count, const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!src || !src_pitch || !width || !height || !comp || !is16bit || !out_offset || !out || !out_len)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "png_encode_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return pencode_batch(src, src_pitch, width, height, comp, is16bit, force_filter, level, count, out_offset, out, out_len, status_host,
                             pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "png_encode_batch_device: out of host memory");
    }
}

// drop-in for stbi_write_png_to_mem (:354): host pixels up through pinned staging (rows packed), one image through the batch path
void* gamut_hip_png_write_to_mem(const void* pixels, int stride_bytes, int x, int y, int n, int* out_len, int is16bit, int force_filter,
                                 int compression_level)
{
    clear_error();
    const int is16 = is16bit ? 1 : 0;
    if (!pixels || !out_len || !pvalid(x, y, n, is16) || compression_level < 0 || compression_level > 10 || pbound(x, y, n, is16) > INT_MAX) {
        set_error(GAMUT_HIP_ERR_INVALID_ARG, "png_write_to_mem: invalid arguments"); return nullptr;
    }
    if (!have_device()) return nullptr;
    const int32_t w = x, hh = y, c = n, s16 = is16, ff = force_filter, lv = compression_level;
    return encode_host_image("png_write_to_mem", HostRows{ pixels, stride_bytes, (size_t)x * n * (is16 ? 2 : 1), y, 1, 0 }, (size_t)pbound(x, y, n, is16), out_len,
        [&](const uint8_t* src, int64_t p, int64_t, int64_t off, uint8_t* d, int64_t* len, hipStream_t st) {
            int status = 0;
            return pencode_batch(&src, &p, &w, &hh, &c, &s16, &ff, &lv, 1, &off, d, len, &status, st);
        });
}

} // extern "C"
