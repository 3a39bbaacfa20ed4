// gif_encode.hip -- GIF encode on the GPU: byte for byte what saveGIF (source/gamut/plugins/gif.d:105-147) gets from msf_gif
// (source/gamut/codecs/msf_gif.d: msf_gif_begin, msf_gif_frame per layer, msf_gif_end), many animations per call, pixels and files in
// HBM.  Arguments, tables and the entry points are in gif_encode_host.hip, which also lists the deliberate deviations.
//
// The number of launches does not depend on the frame count or on how many depths a frame tries:
//
// k_gifenc_census -- 8192 pixels of one frame per workgroup.  The used-colour count that msf_cook_frame's do-while (:204-287) tests is
//   a pure function of the frame's pixels and the depth, so one pass cooks every pixel at ALL 16 depths and sets the used-value bitmaps
//   (2 + 4 + ... + 65536 bits, 16 KiB of LDS), which are then OR-ed into the frame's bitmaps in HBM.  A bit that is already set is not
//   set again, so a flat image costs one broadcast read per lane and depth, not 64 serialised atomics.  The has-transparent flag
//   (alpha < threshold, the same at every depth) is recorded alongside.
// k_gifenc_plan -- one wave per animation walks its frames in order: the start depth from the previous frame's depth and count (:579),
//   down while the chosen bitmap counts >= 256 colours (:287), the frames-compatible flag (:405-406).  This is the only frame-to-frame
//   chain besides the file offsets, and it is a few popcounts per frame.
// k_gifenc_lzw -- one frame per wave, every frame of the batch in one launch.  The wave ranks the chosen bitmap (prefix popcounts ->
//   the translation table :368-396 as "rank of the value", never stored as a table), writes GCE, image descriptor and local colour table,
//   then parses: 64 raw pixels of this frame (and of the previous one when the frames are compatible: its cooked value is recomputed
//   from its pixels at the shared depth, no cooked frame is ever stored) are fetched, cooked and ranked by the lanes, and the greedy
//   parse (:435-459) runs over them as a uniform chain.  The dictionary is the reference's trie in another container: an open-addressed
//   table in LDS keyed by (prefix code, colour) -- the codes assigned depend only on the parse.  Codes go through a 64-bit accumulator
//   into an LDS stage of 1020 bytes, which the lanes store as four 255-byte sub-blocks at a time (:297-316 is plain 255-byte chunking
//   of the code stream: a rollover leaves nothing behind exactly when the stream ends on a sub-block's last bit, which is the
//   `blockBits > 8` test of :466).  Every loop is bounded by the frame's pixel count or the table size, every store by the slot's end.
// k_gifenc_offsets -- one wave per animation: prefix sum of its block lengths -> where each block goes, and the file's length.
// k_gifenc_gather -- 4096 bytes of one block per workgroup, from the frame's scratch slot to the file; the block of the frame in front
//   of a frame with transparent pixels gets disposal 0x09 in its byte 3 here (:411-413), the first block's workgroup adds the 32-byte
//   header (:545-548), the last block's the trailer.
#include "gif_encode_host.hpp"

namespace gamut {
namespace {

constexpr int kWave = 64;
constexpr int kCensusThreads = 256;
constexpr int kGatherThreads = 256;
constexpr uint32_t kHashSlots = 8192;            // >= 2 x the 4094 entries a table can hold
constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kStageDwords = 255;           // 1020 bytes: four sub-blocks

// bit depth of each channel by frame depth (msf_gif.d:185-187): r 0 0 1 1 1 2 2 2 3 3 3 4 4 4 5 5 5, g 0 1 1 1 2 2 2 3 3 3 4 4 4 5 5 5 6,
// b 0 0 0 1 1 1 2 2 2 3 3 3 4 4 4 5 5
__device__ __forceinline__ int rbits_of(int d) { return (d + 1) / 3; }
__device__ __forceinline__ int gbits_of(int d) { return (d + 2) / 3; }
__device__ __forceinline__ int bbits_of(int d) { return d / 3; }

// where depth d's bitmap (2^d bits) starts among a frame's census words: one word each for depths 1..5, then 2, 4, ... 2048
__device__ __forceinline__ uint32_t bitmap_word(int d) { return d <= 5 ? (uint32_t)(d - 1) : 3u + (1u << (d - 5)); }
__device__ __forceinline__ uint32_t bitmap_words(int d) { return d <= 5 ? 1u : 1u << (d - 5); }

// msf_cook_frame's pixel (:259-272; the vector body :229-249 computes the same values: its 16-bit products cannot wrap, 255 * 257 = 65535)
__device__ __forceinline__ uint32_t cook(uint32_t px, uint32_t x, uint32_t y, int depth, int alpha_thr, const GifEncMul& m)
{
    if ((int)(px >> 24) < alpha_thr) return 1u << depth;
    const int rb = rbits_of(depth), gb = gbits_of(depth), bb = bbits_of(depth);
    // the 4 x 4 dither kernel (:194-200), << 12
    const uint32_t kern = (0x5D7F91B36E4CA280ull >> (4 * ((y & 3u) * 4u + (x & 3u)))) & 15u;
    const uint32_t k = kern << 12;
    const uint32_t r = min(65535u, (px & 255u) * m.of(rb) + (k >> rb));
    const uint32_t g = min(65535u, ((px >> 8) & 255u) * m.of(gb) + (k >> gb));
    const uint32_t b = min(65535u, ((px >> 16) & 255u) * m.of(bb) + (k >> bb));
    const uint32_t gmask = ((1u << gb) - 1u) << rb, bmask = ((1u << bb) - 1u) << (rb + gb);
    return ((b >> (16 - depth)) & bmask) | ((g >> (16 - rb - gb)) & gmask) | (r >> (16 - rb));
}

__device__ __forceinline__ uint32_t load_px(const uint8_t* p, bool aligned)
{
    if (aligned) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

__device__ __forceinline__ uint32_t find_frame(const GifEncFrame* frames, uint32_t n, uint32_t unit, bool gather)
{
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if ((gather ? frames[mid].gather0 : frames[mid].census0) <= unit) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(kCensusThreads)
k_gifenc_census(const GifEncAnim* __restrict__ anims, const GifEncFrame* __restrict__ frames, uint32_t n_frames, uint32_t* bitmaps, uint32_t* transp,
                GifEncMul mul)
{
    __shared__ uint32_t bits[kGifCensusWords];
    __shared__ uint32_t any_transparent;
    const uint32_t fi = find_frame(frames, n_frames, blockIdx.x, false);
    const GifEncFrame fr = frames[fi];
    const GifEncAnim a = anims[fr.anim];
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < kGifCensusWords; k += kCensusThreads) bits[k] = 0u;
    if (tid == 0) any_transparent = 0u;
    __syncthreads();
    const uint32_t npx = a.w * a.h, p0 = (blockIdx.x - fr.census0) * kGifCensusPixels;
    const uint32_t p1 = min(npx, p0 + kGifCensusPixels);
    const bool aligned = a.aligned != 0;
    for (uint32_t i = p0 + tid; i < p1; i += kCensusThreads) {
        const uint32_t y = i / a.w, x = i - y * a.w;
        const uint32_t px = load_px(a.src + (int64_t)fr.index * a.layer_off + (int64_t)y * a.pitch + (int64_t)x * 4, aligned);
        if ((int)(px >> 24) < a.alpha_thr) { if (!any_transparent) any_transparent = 1u; continue; }
        for (int d = 1; d <= 16; ++d) {
            const uint32_t v = cook(px, x, y, d, a.alpha_thr, mul);
            const uint32_t w = bitmap_word(d) + (v >> 5), m = 1u << (v & 31u);
            if (!(bits[w] & m)) atomicOr(&bits[w], m);
        }
    }
    __syncthreads();
    uint32_t* g = bitmaps + (size_t)fi * kGifCensusWords;
    for (uint32_t k = tid; k < kGifCensusWords; k += kCensusThreads) { const uint32_t v = bits[k]; if (v) atomicOr(&g[k], v); }
    if (tid == 0 && any_transparent) atomicOr(&transp[fi], 1u);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, kWave);
    return v;
}

__global__ void __launch_bounds__(kWave)
k_gifenc_plan(const GifEncAnim* __restrict__ anims, const uint32_t* __restrict__ bitmaps, const uint32_t* __restrict__ transp, GifEncPlan* plans)
{
    const GifEncAnim a = anims[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    int prev_depth = 0, prev_count = 0;
    for (uint32_t f = 0; f < a.frames; ++f) {
        const uint32_t fi = a.frame0 + f;
        const uint32_t* bm = bitmaps + (size_t)fi * kGifCensusWords;
        int d = min(a.max_depth, prev_depth + 160 / max(1, prev_count));                      // :579
        int count = 0;
        for (int tries = 0; tries < 16; ++tries) {                                             // :204-287
            const uint32_t w0 = bitmap_word(d), nw = bitmap_words(d);
            uint32_t c = 0;
            for (uint32_t k = lane; k < nw; k += kWave) c += (uint32_t)__popc(bm[w0 + k]);
            count = (int)wave_sum(c);
            if (count >= 256 && d > 1) --d; else break;
        }
        const int has_t = transp[fi] ? 1 : 0;
        if (lane == 0) {
            GifEncPlan p{};
            p.depth = d; p.count = count; p.has_transparent = has_t;
            p.compatible = (f > 0 && d == prev_depth && !has_t) ? 1 : 0;                        // :405-406 (each depth has its own bit split)
            plans[fi] = p;
        }
        prev_depth = d; prev_count = count;
    }
}

__global__ void __launch_bounds__(kWave)
k_gifenc_lzw(const GifEncAnim* __restrict__ anims, const GifEncFrame* __restrict__ frames, const uint32_t* __restrict__ bitmaps, GifEncPlan* plans,
             uint8_t* slots, GifEncMul mul)
{
    __shared__ uint32_t dict[kHashSlots];
    __shared__ uint32_t bm[2048];
    __shared__ uint8_t  prefix[2048];
    __shared__ uint32_t stage[kStageDwords + 1];
    __shared__ uint32_t lane_sum[kWave];

    const uint32_t fi = blockIdx.x, lane = threadIdx.x;
    const GifEncFrame fr = frames[fi];
    const GifEncAnim a = anims[fr.anim];
    const GifEncPlan pl = plans[fi];
    const int depth = pl.depth;
    const bool compatible = pl.compatible != 0, aligned = a.aligned != 0;
    const uint32_t npx = a.w * a.h;
    const uint32_t table_bits = max(2u, (uint32_t)(32 - __clz(max(pl.count, 1)) ));             // :401 (msf_bit_log(0) is 1)
    const uint32_t table_size = 1u << table_bits;
    // the block starts so far into its slot that the sub-block chain starts on a multiple of 4
    const uint32_t head = 18u + 3u * table_size + 1u, pad = (4u - (head & 3u)) & 3u;
    uint8_t* blk = slots + fr.slot + pad;
    const uint32_t cap = fr.slot_cap;
    bool overflow = false;
    auto put = [&](uint32_t at, uint32_t v) { if (at < cap) blk[at] = (uint8_t)v; else overflow = true; };

    // ---- rank the chosen bitmap: prefix[w] = used values below word w
    const uint32_t nw = bitmap_words(depth), per = (nw + kWave - 1) / kWave;
    {
        const uint32_t* g = bitmaps + (size_t)fi * kGifCensusWords + bitmap_word(depth);
        uint32_t s = 0;
        for (uint32_t k = 0; k < per; ++k) { const uint32_t w = lane * per + k; if (w < nw) { const uint32_t v = g[w]; bm[w] = v; s += (uint32_t)__popc(v); } }
        lane_sum[lane] = s;
    }
    // ---- GCE + image descriptor (:408-418), zeroed colour table (:366, :422), LZW minimum code size (:424)
    if (lane < 18) {
        uint32_t v = 0;
        switch (lane) {
            case 0: v = 0x21; break; case 1: v = 0xF9; break; case 2: v = 0x04; break; case 3: v = 0x05; break;
            case 4: v = (uint32_t)a.centis & 255u; break; case 5: v = ((uint32_t)a.centis >> 8) & 255u; break;
            case 8: v = 0x2C; break;
            case 13: v = a.w & 255u; break; case 14: v = a.w >> 8; break; case 15: v = a.h & 255u; break; case 16: v = a.h >> 8; break;
            case 17: v = 0x80u | (table_bits - 1u); break;
            default: break;
        }
        put(lane, v);
    }
    for (uint32_t k = lane; k < 3u * table_size; k += kWave) put(18u + k, 0u);
    if (lane == 0) put(18u + 3u * table_size, table_bits);
    for (uint32_t k = lane; k < kHashSlots; k += kWave) dict[k] = kEmpty;
    __syncthreads();
    {
        uint32_t base = 0;
        for (uint32_t l = 0; l < lane; ++l) base += lane_sum[l];
        const int rb = rbits_of(depth), gb = gbits_of(depth), bb = bbits_of(depth);
        for (uint32_t k = 0; k < per; ++k) {
            const uint32_t w = lane * per + k;
            if (w >= nw) break;
            prefix[w] = (uint8_t)base;
            uint32_t v = bm[w];
            while (v) {
                const uint32_t bit = (uint32_t)__ffs((int)v) - 1u; v &= v - 1u;
                const uint32_t val = w * 32u + bit, idx = ++base;                               // ranks from 1 in ascending cooked value
                if (idx > 255u) break;                                                          // (count < 256: cannot happen)
                uint32_t r = val & ((1u << rb) - 1u), g = (val >> rb) & ((1u << gb) - 1u), b = val >> (rb + gb);
                r <<= 8 - rb; g <<= 8 - gb; b <<= 8 - bb;                                       // bit replication (:383-388)
                r = rb ? (r | r >> rb | r >> (rb * 2) | r >> (rb * 3)) : 0u;
                g = gb ? (g | g >> gb | g >> (gb * 2) | g >> (gb * 3)) : 0u;
                b = bb ? (b | b >> bb | b >> (bb * 2) | b >> (bb * 3)) : 0u;
                put(18u + 3u * idx, r & 255u); put(18u + 3u * idx + 1u, g & 255u); put(18u + 3u * idx + 2u, b & 255u);
            }
        }
    }
    __syncthreads();

    // ---- the code stream
    uint32_t out_pos = head;                                                                   // uniform
    uint64_t acc = 0; uint32_t nbits = 0, sw = 0;                                              // uniform
    auto flush_full = [&](uint32_t nblocks) {                                                  // nblocks * 255 staged bytes -> nblocks sub-blocks
        __syncthreads();
        const uint8_t* sb = reinterpret_cast<const uint8_t*>(stage);
        for (uint32_t k = lane; k < nblocks * 256u; k += kWave) {
            const uint32_t b = k >> 8, r = k & 255u;
            put(out_pos + k, r == 0 ? 255u : sb[b * 255u + r - 1u]);
        }
        out_pos += nblocks * 256u;
        __syncthreads();
    };
    auto emit = [&](uint32_t code, uint32_t width) {
        acc |= (uint64_t)code << nbits; nbits += width;
        if (nbits >= 32) {
            if (lane == 0) stage[sw] = (uint32_t)acc;
            acc >>= 32; nbits -= 32; ++sw;
            if (sw == kStageDwords) { flush_full(4); sw = 0; }
        }
    };
    auto bit_log = [](uint32_t v) -> uint32_t { return v ? 32u - (uint32_t)__clz((int)v) : 1u; };

    uint32_t len = table_size + 2u;                                                            // :325-330
    uint32_t resets = 0;
    emit(table_size, bit_log(len - 1u));                                                       // the clear code first (:433)
    uint32_t last = 0;
    const uint32_t transparent_value = 1u << depth;
    for (uint32_t base = 0; base < npx; base += kWave) {
        // colour index of pixel base + lane
        uint32_t colour = 0;
        const uint32_t i = base + lane;
        if (i < npx) {
            const uint32_t y = i / a.w, x = i - y * a.w;
            const uint8_t* p = a.src + (int64_t)fr.index * a.layer_off + (int64_t)y * a.pitch + (int64_t)x * 4;
            const uint32_t v = cook(load_px(p, aligned), x, y, depth, a.alpha_thr, mul);
            bool same = false;
            if (compatible) same = cook(load_px(p - a.layer_off, aligned), x, y, depth, a.alpha_thr, mul) == v;        // :439
            if (!same && v != transparent_value)
                colour = (uint32_t)prefix[v >> 5] + (uint32_t)__popc(bm[v >> 5] & ((1u << (v & 31u)) - 1u)) + 1u;
        }
        const uint32_t n = min((uint32_t)kWave, npx - base);
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)colour, (int)j);
            if (base + j == 0) { last = c; continue; }                                         // :435
            const uint32_t key = last << 8 | c;
            uint32_t h = (key * 0x9E3779B1u) >> 19;
            uint32_t code = kEmpty;
            for (uint32_t probes = 0; probes < kHashSlots; ++probes) {
                const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)dict[h]);
                if (e == kEmpty) break;
                if ((e >> 12) == key) { code = e & 4095u; break; }
                h = (h + 1u) & (kHashSlots - 1u);
            }
            if (code != kEmpty) { last = code; continue; }
            const uint32_t code_bits = bit_log(len - 1u);                                      // :443-455
            emit(last, code_bits);
            if (len > 4095u) {
                emit(table_size, code_bits);
                __syncthreads();
                for (uint32_t k = lane; k < kHashSlots; k += kWave) dict[k] = kEmpty;
                __syncthreads();
                len = table_size + 2u; ++resets;
            } else {
                if (lane == 0) dict[h] = key << 12 | len;
                ++len;
            }
            last = c;
        }
    }
    emit(last, min(12u, bit_log(len - 1u)));                                                   // :462-463
    emit(table_size + 1u, min(12u, bit_log(len)));
    if (nbits) { if (lane == 0) stage[sw] = (uint32_t)acc; }
    const uint32_t nbytes = sw * 4u + (nbits + 7u) / 8u;                                       // <= 1020
    const uint32_t full = nbytes / 255u, rem = nbytes - full * 255u;
    flush_full(full);                                                                          // (also orders the stage's last dword)
    if (rem) {                                                                                 // :466-470
        const uint8_t* sb = reinterpret_cast<const uint8_t*>(stage);
        for (uint32_t k = lane; k < rem + 1u; k += kWave) put(out_pos + k, k == 0 ? rem : sb[full * 255u + k - 1u]);
        out_pos += rem + 1u;
    }
    if (lane == 0) put(out_pos, 0u);                                                           // :471
    out_pos += 1u;
    const bool any_overflow = __any(overflow);
    if (lane == 0) {
        plans[fi].block_len = any_overflow ? 0u : out_pos;
        plans[fi].block_pad = pad;
        plans[fi].overflow = any_overflow ? 1u : 0u;
        plans[fi].resv = resets;
    }
}

__global__ void __launch_bounds__(kWave)
k_gifenc_offsets(const GifEncAnim* __restrict__ anims, GifEncPlan* plans, int64_t* total_len)
{
    const GifEncAnim a = anims[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    uint64_t running = 32;
    uint32_t bad = 0;
    for (uint32_t f0 = 0; f0 < a.frames; f0 += kWave) {
        const uint32_t f = f0 + lane;
        const uint32_t l = f < a.frames ? plans[a.frame0 + f].block_len : 0u;
        if (f < a.frames && plans[a.frame0 + f].overflow) bad = 1u;
        uint64_t incl = l;                                                                     // (64 blocks of up to 0.8 GB: the sums need 64 bits)
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)incl, o, kWave), hi = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), o, kWave);
            if ((int)lane >= o) incl += (uint64_t)hi << 32 | lo;
        }
        if (f < a.frames) plans[a.frame0 + f].file_off = running + incl - l;
        running += (uint64_t)(uint32_t)__shfl((int)(uint32_t)(incl >> 32), kWave - 1, kWave) << 32 | (uint32_t)__shfl((int)(uint32_t)incl, kWave - 1, kWave);
    }
    const bool any_bad = __any(bad);
    if (lane == 0) total_len[blockIdx.x] = any_bad ? -1 : (int64_t)(running + 1);
}

__global__ void __launch_bounds__(kGatherThreads)
k_gifenc_gather(const GifEncAnim* __restrict__ anims, const GifEncFrame* __restrict__ frames, uint32_t n_frames, const GifEncPlan* __restrict__ plans,
                const uint8_t* __restrict__ slots, const int64_t* __restrict__ total_len, uint8_t* out)
{
    const uint32_t fi = find_frame(frames, n_frames, blockIdx.x, true);
    const GifEncFrame fr = frames[fi];
    const GifEncAnim a = anims[fr.anim];
    const int64_t total = total_len[fr.anim];
    if (total < 0) return;                                                                     // (a frame overflowed its slot: the file is left alone)
    const GifEncPlan pl = plans[fi];
    const uint32_t tid = threadIdx.x, chunk = blockIdx.x - fr.gather0;
    uint8_t* file = out + a.out_off;
    if (chunk == 0) {
        if (fr.index == 0 && tid < 32) {                                                       // :545-548
            const char* tail = "\x21\xFF\x0BNETSCAPE2.0\x03\x01";
            uint32_t v = 0;
            if (tid < 6) v = (uint8_t)"GIF89a"[tid];
            else if (tid == 6) v = a.w & 255u; else if (tid == 7) v = a.w >> 8; else if (tid == 8) v = a.h & 255u; else if (tid == 9) v = a.h >> 8;
            else if (tid == 10) v = 0x70;
            else if (tid >= 13 && tid < 29) v = (uint8_t)tail[tid - 13];
            file[tid] = (uint8_t)v;
        }
        if (fr.index + 1 == a.frames && tid == 0) file[total - 1] = 0x3B;
    }
    const uint32_t b0 = chunk * kGifGatherBytes;
    if (b0 >= pl.block_len) return;
    const uint32_t b1 = min(pl.block_len, b0 + kGifGatherBytes);
    const bool next_transparent = fr.index + 1 < a.frames && plans[fi + 1].has_transparent;    // :411-413
    const uint8_t* s = slots + fr.slot + pl.block_pad;
    uint8_t* d = file + pl.file_off;
    for (uint32_t k = b0 + tid; k < b1; k += kGatherThreads) {
        uint8_t v = s[k];
        if (k == 3 && next_transparent) v = 0x09;
        d[k] = v;
    }
}

} // namespace

int gifenc_launch(const GifEncAnim* anims, int n_anim, const GifEncFrame* frames, uint32_t n_frames, uint32_t census_units, uint32_t gather_units,
                  uint32_t* bitmaps, uint32_t* transp, GifEncPlan* plans, uint8_t* slots, int64_t* total_len, uint8_t* out, const GifEncMul& mul,
                  hipStream_t stream, KernelTimer<6>& timer)
{
    timer.mark(stream);
    hipLaunchKernelGGL(k_gifenc_census, dim3(census_units), dim3(kCensusThreads), 0, stream, anims, frames, n_frames, bitmaps, transp, mul);
    if (int rc = launch_status("gifenc_census")) return rc;
    timer.mark(stream);
    hipLaunchKernelGGL(k_gifenc_plan, dim3((uint32_t)n_anim), dim3(kWave), 0, stream, anims, (const uint32_t*)bitmaps, (const uint32_t*)transp, plans);
    if (int rc = launch_status("gifenc_plan")) return rc;
    timer.mark(stream);
    hipLaunchKernelGGL(k_gifenc_lzw, dim3(n_frames), dim3(kWave), 0, stream, anims, frames, (const uint32_t*)bitmaps, plans, slots, mul);
    if (int rc = launch_status("gifenc_lzw")) return rc;
    timer.mark(stream);
    hipLaunchKernelGGL(k_gifenc_offsets, dim3((uint32_t)n_anim), dim3(kWave), 0, stream, anims, plans, total_len);
    if (int rc = launch_status("gifenc_offsets")) return rc;
    timer.mark(stream);
    hipLaunchKernelGGL(k_gifenc_gather, dim3(gather_units), dim3(kGatherThreads), 0, stream, anims, frames, n_frames, (const GifEncPlan*)plans,
                       (const uint8_t*)slots, (const int64_t*)total_len, out);
    if (int rc = launch_status("gifenc_gather")) return rc;
    timer.mark(stream);
    return GAMUT_HIP_OK;
}

} // namespace gamut
